// Step glue that used to run as stock ATen kernels on the hot path (VERDICT r1 "weak 5"): the
// cross-entropy reduction, BatchNorm running statistics, the weight-normed k3 conv weights and their
// layouts, the processor's output blend, segmented gradient accumulation.  Each entry names the
// reference op it replaces.
#include "common.h"

namespace asrx {

// ---------------------------------------------------------------------------- cross entropy
// F.cross_entropy(logits, labels, ignore_index=0) (model.py:670), one logits row per workgroup in a
// single pass: each thread keeps an online (max, sum exp) pair, the pairs are merged, and the
// target logit is picked on the way.  loss_r[r] = lse - z[y] (0 for ignored rows).
__global__ __launch_bounds__(256) void ce_fwd1_kernel(const float* __restrict__ z, const int64_t* __restrict__ labels,
                                                      float* __restrict__ loss, float* __restrict__ lse, int64_t V) {
  __shared__ float rm[4], rs[4];
  const int64_t r = blockIdx.x;
  const float* zr = z + r * V;
  const int64_t y = labels[r];
  float m = -INFINITY, s = 0.f;
  const float4* z4 = reinterpret_cast<const float4*>(zr);
  const int64_t V4 = (V % 4 == 0 && ((uintptr_t)zr & 15) == 0) ? V / 4 : 0;
  auto add = [&](float v) {
    if (v > m) {
      s = s * __expf(m - v) + 1.f;
      m = v;
    } else {
      s += __expf(v - m);
    }
  };
  for (int64_t j = threadIdx.x; j < V4; j += 256) {
    const float4 v = z4[j];
    add(v.x);
    add(v.y);
    add(v.z);
    add(v.w);
  }
  for (int64_t j = 4 * V4 + threadIdx.x; j < V; j += 256) add(zr[j]);
  // merge (m, s) across the wave, then across the 4 waves
  for (int o = 32; o >= 1; o >>= 1) {
    const float mo = __shfl_xor(m, o), so = __shfl_xor(s, o);
    const float mn = fmaxf(m, mo);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
    m = mn;
  }
  if ((threadIdx.x & 63) == 0) {
    rm[threadIdx.x >> 6] = m;
    rs[threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3])), S = 0.f;
    for (int w = 0; w < 4; ++w) S += rs[w] * __expf(rm[w] - M);
    const float l = M + logf(S);
    lse[r] = l;
    // a label outside [0, V) (the reference's F.cross_entropy raises) makes the loss NaN instead of
    // reading outside the row
    loss[r] = (y < 0 || y >= V) ? __builtin_nanf("") : (y == 0 ? 0.f : l - zr[y]);
  }
}

// The cross entropy from the fused logits GEMM's partials (asrx_gemm_wn_ce): per row, merge the
// nparts (max, sum exp) pairs of its column tiles into the log-sum-exp and read the label's bf16 logit
// (2 bytes) -- the 40000-wide row itself is not re-read.  One wave per row, 4 rows per workgroup.
__global__ __launch_bounds__(256) void ce_part_fwd_kernel(const float2* __restrict__ part, int nparts,
                                                          const unsigned short* __restrict__ zb,
                                                          const float* __restrict__ zf,
                                                          const int64_t* __restrict__ labels, float* __restrict__ loss,
                                                          float* __restrict__ lse, int64_t rows, int64_t V) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  float m = -INFINITY, s = 0.f;
  for (int j = lane; j < nparts; j += 64) {
    const float2 v = part[r * nparts + j];
    const float mn = fmaxf(m, v.x);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (v.x == -INFINITY ? 0.f : v.y * __expf(v.x - mn));
    m = mn;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const float mo = __shfl_xor(m, o), so = __shfl_xor(s, o);
    const float mn = fmaxf(m, mo);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
    m = mn;
  }
  if (lane == 0) {
    const int64_t y = labels[r];
    const float l = m + logf(s);
    lse[r] = l;
    float lr = 0.f;
    if (y < 0 || y >= V) lr = __builtin_nanf("");
    else if (y != 0) lr = l - (zf ? zf[r * V + y] : __builtin_bit_cast(float, (uint32_t)zb[r * V + y] << 16));
    loss[r] = lr;
  }
}

// The rows of the logits-free head (asrx_gemm_wn_head) from its per-tile partials: the (max, sum exp) pairs
// merge in ce_part_fwd_kernel's order, so lse is the number the fused cross entropy gives; pred is the column
// of the global max, the lowest among the tiles (and, within one, the columns) that hold it -- torch.argmax's
// rule; column 0 when no tile has a value above -inf.  With labels: loss_r = lse - zlab (0 for label 0, NaN
// for a label outside [0, V)).  labels null: pred only (the decode form).  One wave per row.
__global__ __launch_bounds__(256) void head_merge_kernel(const float2* __restrict__ part, const int* __restrict__ idx,
                                                         int nparts, const float* __restrict__ zlab,
                                                         const int64_t* __restrict__ labels, int64_t* __restrict__ pred,
                                                         float* __restrict__ loss, float* __restrict__ lse, int64_t rows,
                                                         int64_t V) {
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= rows) return;
  float m = -INFINITY, s = 0.f;
  int ix = 0x7fffffff;
  for (int j = lane; j < nparts; j += 64) {
    const float2 v = part[r * nparts + j];
    const int iv = idx[r * nparts + j];
    if (v.x > m || (v.x == m && iv < ix)) ix = iv;
    const float mn = fmaxf(m, v.x);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (v.x == -INFINITY ? 0.f : v.y * __expf(v.x - mn));
    m = mn;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    const float mo = __shfl_xor(m, o), so = __shfl_xor(s, o);
    const int io = __shfl_xor(ix, o);
    if (mo > m || (mo == m && io < ix)) ix = io;
    const float mn = fmaxf(m, mo);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (mo == -INFINITY ? 0.f : so * __expf(mo - mn));
    m = mn;
  }
  if (lane == 0) {
    pred[r] = (ix >= 0 && ix < V) ? ix : 0;
    if (labels) {
      const int64_t y = labels[r];
      const float l = m + logf(s);
      lse[r] = l;
      float lr = 0.f;
      if (y < 0 || y >= V) lr = __builtin_nanf("");
      else if (y != 0) lr = l - zlab[r];
      loss[r] = lr;
    }
  }
}

// correct = #{rows: label != 0 and pred == label} and count = #{rows: label != 0} (numerator and denominator of
// asrx.metrics.evaluate_loader's token accuracy): integer partial counts summed by one workgroup in a fixed
// order.  count replaces ce_reduce_kernel's max(#, 1) -- a backward's divisor, which evaluation has no use for.
__global__ __launch_bounds__(1024) void head_count_kernel(const int64_t* __restrict__ pred,
                                                          const int64_t* __restrict__ labels, int64_t rows,
                                                          int64_t* __restrict__ correct, float* __restrict__ count) {
  __shared__ int red[2][16];
  int c = 0, n = 0;
  for (int64_t r = threadIdx.x; r < rows; r += 1024) {
    const int64_t y = labels[r];
    n += y != 0 ? 1 : 0;
    c += (y != 0 && pred[r] == y) ? 1 : 0;
  }
  for (int o = 32; o >= 1; o >>= 1) {
    c += __shfl_xor(c, o);
    n += __shfl_xor(n, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = c;
    red[1][threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t tc = 0, tn = 0;
    for (int i = 0; i < 16; ++i) {
      tc += red[0][i];
      tn += red[1][i];
    }
    correct[0] = tc;
    count[0] = (float)tn;
  }
}

// dz = (g / count) (softmax(z) - onehot(y)) from the bf16 logits, stored bf16 (it only feeds the two
// gradient GEMMs, which round their operands to bf16 anyway).  One row per workgroup, 8 logits per
// 16-byte load.
__global__ __launch_bounds__(256) void ce_bwd_bf16_kernel(const unsigned short* __restrict__ zb,
                                                          const int64_t* __restrict__ labels,
                                                          const float* __restrict__ lse, const float* __restrict__ g,
                                                          const float* __restrict__ count,
                                                          unsigned short* __restrict__ dzb, int64_t V) {
  const int64_t r = blockIdx.x;
  const int64_t y = labels[r];
  const bool bad = y < 0 || y >= V;
  const float sc = bad ? __builtin_nanf("") : (y == 0 ? 0.f : g[0] / count[0]);
  const float l = lse[r];
  const unsigned short* zr = zb + r * V;
  unsigned short* dr = dzb + r * V;
  auto f = [&](unsigned short h, int64_t j) {
    const float v = __builtin_bit_cast(float, (uint32_t)h << 16);
    return __builtin_bit_cast(unsigned short, (__bf16)(sc * (__expf(v - l) - (j == y ? 1.f : 0.f))));
  };
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const bool vec = V % 8 == 0 && (((uintptr_t)zr | (uintptr_t)dr) & 15) == 0;
  const int64_t V8 = vec ? V / 8 : 0;
  for (int64_t j = threadIdx.x; j < V8; j += 256) {
    const u32x4 in = reinterpret_cast<const u32x4*>(zr)[j];
    u32x4 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned short lo = f((unsigned short)(in[q] & 0xFFFF), 8 * j + 2 * q);
      const unsigned short hi = f((unsigned short)(in[q] >> 16), 8 * j + 2 * q + 1);
      out[q] = (unsigned)lo | ((unsigned)hi << 16);
    }
    reinterpret_cast<u32x4*>(dr)[j] = out;
  }
  for (int64_t j = 8 * V8 + threadIdx.x; j < V; j += 256) dr[j] = f(zr[j], j);
}

// As ce_bwd_bf16_kernel from fp32 logits (the boundary's fp32 logits, asrx_gemm_wn_ce_f32): dz stored
// bf16, 8 logits per two 16-byte loads.
__global__ __launch_bounds__(256) void ce_bwd_f32in_kernel(const float* __restrict__ zf,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse, const float* __restrict__ g,
                                                           const float* __restrict__ count,
                                                           unsigned short* __restrict__ dzb, int64_t V) {
  const int64_t r = blockIdx.x;
  const int64_t y = labels[r];
  const bool bad = y < 0 || y >= V;
  const float sc = bad ? __builtin_nanf("") : (y == 0 ? 0.f : g[0] / count[0]);
  const float l = lse[r];
  const float* zr = zf + r * V;
  unsigned short* dr = dzb + r * V;
  auto f = [&](float v, int64_t j) {
    return __builtin_bit_cast(unsigned short, (__bf16)(sc * (__expf(v - l) - (j == y ? 1.f : 0.f))));
  };
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const bool vec = V % 8 == 0 && (((uintptr_t)zr | (uintptr_t)dr) & 15) == 0;
  const int64_t V8 = vec ? V / 8 : 0;
  for (int64_t j = threadIdx.x; j < V8; j += 256) {
    const float4 a = reinterpret_cast<const float4*>(zr)[2 * j], b = reinterpret_cast<const float4*>(zr)[2 * j + 1];
    const int64_t c = 8 * j;
    u32x4 out;
    out[0] = (unsigned)f(a.x, c) | ((unsigned)f(a.y, c + 1) << 16);
    out[1] = (unsigned)f(a.z, c + 2) | ((unsigned)f(a.w, c + 3) << 16);
    out[2] = (unsigned)f(b.x, c + 4) | ((unsigned)f(b.y, c + 5) << 16);
    out[3] = (unsigned)f(b.z, c + 6) | ((unsigned)f(b.w, c + 7) << 16);
    reinterpret_cast<u32x4*>(dr)[j] = out;
  }
  for (int64_t j = 8 * V8 + threadIdx.x; j < V; j += 256) dr[j] = f(zr[j], j);
}

// loss = sum_r loss_r / #{labels != 0} (NaN when every label is ignored, as F.cross_entropy's mean,
// model.py:670); count = max(#, 1) kept for the backward (ignored rows get a zero gradient).  One workgroup.
__global__ __launch_bounds__(1024) void ce_reduce_kernel(const float* __restrict__ loss_r, const int64_t* __restrict__ labels,
                                                         int64_t rows, float* __restrict__ loss, float* __restrict__ count) {
  __shared__ float red[16];
  float s = 0.f, c = 0.f;
  for (int64_t r = threadIdx.x; r < rows; r += 1024) {
    s += loss_r[r];
    c += labels[r] != 0 ? 1.f : 0.f;
  }
  s = block_sum<1024>(s, red);
  c = block_sum<1024>(c, red);
  if (threadIdx.x == 0) {
    loss[0] = c > 0.f ? s / c : __builtin_nanf("");
    count[0] = fmaxf(c, 1.f);
  }
}

// dz = (g / count) (softmax(z) - onehot(y)) for non-ignored rows, 0 otherwise; g = d loss (device
// scalar, so nothing syncs with the host).  dz may alias z (in place).
__global__ __launch_bounds__(256) void ce_bwd2_kernel(const float* z, const int64_t* __restrict__ labels,
                                                      const float* __restrict__ lse, const float* __restrict__ g,
                                                      const float* __restrict__ count, float* dz, int64_t V) {
  const int64_t r = blockIdx.x;
  const int64_t y = labels[r];
  const float sc = (y < 0 || y >= V) ? __builtin_nanf("") : ((y == 0) ? 0.f : g[0] / count[0]);
  const float l = lse[r];
  const float* zr = z + r * V;
  float* dr = dz + r * V;
  if (V % 4 == 0 && (((uintptr_t)zr | (uintptr_t)dr) & 15) == 0) {
    const float4* z4 = reinterpret_cast<const float4*>(zr);
    float4* d4 = reinterpret_cast<float4*>(dr);
    for (int64_t j = threadIdx.x; j < V / 4; j += 256) {
      const float4 v = z4[j];
      float4 o;
      o.x = sc * (__expf(v.x - l) - (4 * j + 0 == y ? 1.f : 0.f));
      o.y = sc * (__expf(v.y - l) - (4 * j + 1 == y ? 1.f : 0.f));
      o.z = sc * (__expf(v.z - l) - (4 * j + 2 == y ? 1.f : 0.f));
      o.w = sc * (__expf(v.w - l) - (4 * j + 3 == y ? 1.f : 0.f));
      d4[j] = o;
    }
  } else {
    for (int64_t j = threadIdx.x; j < V; j += 256) dr[j] = sc * (__expf(zr[j] - l) - (j == y ? 1.f : 0.f));
  }
}

// ---------------------------------------------------------------------------- BatchNorm running stats
// nn.BatchNorm1d's running-statistic update (ConvLite.bn, model.py:101) from the per-clip statistics of
// the batch-1 semantics (asrx.model.ConvLite._update_running): rm = (1-m) rm + m mean_b(mean),
// rv = (1-m) rv + m mean_b((1/rstd^2 - eps) T/(T-1)); num_batches_tracked += 1.
__global__ void bn_running_kernel(const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ rm,
                                  float* __restrict__ rv, int64_t* __restrict__ nbt, int B, int C, float eps,
                                  float unbias, float mom) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    float sm = 0.f, sv = 0.f;
    for (int b = 0; b < B; ++b) {
      const float r = rstd[b * C + c];
      sm += mean[b * C + c];
      sv += (1.f / (r * r) - eps) * unbias;
    }
    rm[c] = (1.f - mom) * rm[c] + mom * (sm / B);
    rv[c] = (1.f - mom) * rv[c] + mom * (sv / B);
  }
  if (c == 0 && nbt) nbt[0] += 1;
}

// The same update from statistics over per-sample lengths (asrx_bn_silu_lens_fwd): sample b's variance is unbiased
// by T_b / (T_b - 1), T_b = clamp(lens[b], 0, T); a sample without rows adds mean 0 and variance 0.
__global__ void bn_running_lens_kernel(const float* __restrict__ mean, const float* __restrict__ rstd,
                                       float* __restrict__ rm, float* __restrict__ rv, int64_t* __restrict__ nbt,
                                       const int32_t* __restrict__ lens, int B, int C, int T, float eps, float mom) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) {
    float sm = 0.f, sv = 0.f;
    for (int b = 0; b < B; ++b) {
      const int Tb = min(max(lens[b], 0), T);
      if (Tb == 0) continue;
      const float unbias = (float)Tb / (float)max(Tb - 1, 1);
      const float r = rstd[b * C + c];
      sm += mean[b * C + c];
      sv += (1.f / (r * r) - eps) * unbias;
    }
    rm[c] = (1.f - mom) * rm[c] + mom * (sm / B);
    rv[c] = (1.f - mom) * rv[c] + mom * (sv / B);
  }
  if (c == 0 && nbt) nbt[0] += 1;
}

// eval-mode BatchNorm's rstd = rsqrt(running_var + eps)
__global__ void rsqrt_eps_kernel(const float* __restrict__ v, float* __restrict__ out, int n, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rsqrtf(v[i] + eps);
}

// ---------------------------------------------------------------------------- k3 conv weights
// weight_norm(Conv1d(C, C, 3)) (model.py:140) and the stem Conv1d(mels, D, 3): W = g v / |v|_o (norm over
// (Ci, 3) per output channel; g null = plain weight).  Written straight into the layouts the
// implicit-im2col GEMMs read: Wt (Co, 3 Ci) k-major (Wt[o, k Ci + i] = W[o, i, k]) for the forward and
// Wf (Ci, 3 Co) flipped (Wf[i, k Co + o] = W[o, i, 2 - k]) for the input gradient; each fp32 and/or bf16
// (any pointer may be null).  nrm[o] = |v_o| for the backward.  One workgroup per output channel.
__global__ __launch_bounds__(256) void conv3_weight_kernel(const float* __restrict__ g, const float* __restrict__ v,
                                                           int Co, int Ci, float* __restrict__ Wt,
                                                           unsigned short* __restrict__ Wtb, float* __restrict__ Wf,
                                                           unsigned short* __restrict__ Wfb, float* __restrict__ nrm) {
  __shared__ float red[4];
  const int o = blockIdx.x;
  const float* vo = v + (int64_t)o * Ci * 3;
  float sc = 1.f;
  if (g) {
    float s = 0.f;
    for (int j = threadIdx.x; j < 3 * Ci; j += 256) s += vo[j] * vo[j];
    const float n = sqrtf(block_sum<256>(s, red));
    sc = g[o] / n;
    if (threadIdx.x == 0 && nrm) nrm[o] = n;
  }
  for (int j = threadIdx.x; j < 3 * Ci; j += 256) {
    const int i = j / 3, k = j % 3;
    const float w = vo[j] * sc;
    const __bf16 h = (__bf16)w;
    const int64_t t = (int64_t)o * 3 * Ci + k * Ci + i;
    const int64_t f = (int64_t)i * 3 * Co + (2 - k) * Co + o;
    if (Wt) Wt[t] = w;
    if (Wtb) Wtb[t] = __builtin_bit_cast(unsigned short, h);
    if (Wf) Wf[f] = w;
    if (Wfb) Wfb[f] = __builtin_bit_cast(unsigned short, h);
  }
}

// Backward of conv3_weight from the k-major weight gradient dWt (Co, 3 Ci): with g null,
// dv += dW; else W = g v / n: dg += sum dW v / n, dv += (g / n) (dW - (sum dW v) v / n^2).
__global__ __launch_bounds__(256) void conv3_weight_bwd_kernel(const float* __restrict__ dWt, const float* __restrict__ g,
                                                               const float* __restrict__ v, const float* __restrict__ nrm,
                                                               int Co, int Ci, float* __restrict__ dg,
                                                               float* __restrict__ dv) {
  __shared__ float red[4];
  const int o = blockIdx.x;
  const float* vo = v + (int64_t)o * Ci * 3;
  const float* dw = dWt + (int64_t)o * 3 * Ci;
  float* dvo = dv + (int64_t)o * Ci * 3;
  if (!g) {
    for (int j = threadIdx.x; j < 3 * Ci; j += 256) dvo[j] += dw[(j % 3) * Ci + j / 3];
    return;
  }
  float s = 0.f;
  for (int j = threadIdx.x; j < 3 * Ci; j += 256) s += dw[(j % 3) * Ci + j / 3] * vo[j];
  s = block_sum<256>(s, red);
  const float n = nrm[o], go = g[o];
  if (threadIdx.x == 0) dg[o] += s / n;
  const float a = go / n, b = s / (n * n);
  for (int j = threadIdx.x; j < 3 * Ci; j += 256) dvo[j] += a * (dw[(j % 3) * Ci + j / 3] - b * vo[j]);
}

// ---------------------------------------------------------------------------- processor blend
// out = s d + (1 - s) g, s = sigmoid(blend) (model.py:628); backward dd = s go, dg = (1 - s) go and
// d blend += s (1 - s) sum go (d - g) (accumulated into blend's gradient).
__global__ void blend_fwd_kernel(const float4* __restrict__ d, const float4* __restrict__ g, const float* __restrict__ blend,
                                 float4* __restrict__ out, int64_t n4) {
  const float s = 1.f / (1.f + __expf(-blend[0]));
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = d[i], b = g[i];
    out[i] = make_float4(s * a.x + (1.f - s) * b.x, s * a.y + (1.f - s) * b.y, s * a.z + (1.f - s) * b.z,
                         s * a.w + (1.f - s) * b.w);
  }
}

__global__ __launch_bounds__(256) void blend_bwd_kernel(const float4* __restrict__ go, const float4* __restrict__ d,
                                                        const float4* __restrict__ g, const float* __restrict__ blend,
                                                        float4* __restrict__ dd, float4* __restrict__ dg,
                                                        float* __restrict__ dblend, int64_t n4) {
  __shared__ float red[4];
  const float s = 1.f / (1.f + __expf(-blend[0]));
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 u = go[i], a = d[i], b = g[i];
    if (dd) dd[i] = make_float4(s * u.x, s * u.y, s * u.z, s * u.w);
    if (dg) dg[i] = make_float4((1.f - s) * u.x, (1.f - s) * u.y, (1.f - s) * u.z, (1.f - s) * u.w);
    acc += u.x * (a.x - b.x) + u.y * (a.y - b.y) + u.z * (a.z - b.z) + u.w * (a.w - b.w);
  }
  acc = block_sum<256>(acc, red);
  if (threadIdx.x == 0 && dblend) atomicAdd(dblend, s * (1.f - s) * acc);
}

// ---------------------------------------------------------------------------- segmented accumulate
// dst_k[i] += src[k n + i] (k < nseg <= 3): the gradient of a concatenated weight (tgate's Linear(D, 3D)
// of three Linear(D, D), model.py:530) landing in each part's own gradient buffer.
__global__ void add_segments_kernel(const float* __restrict__ src, int64_t n, float* __restrict__ d0,
                                    float* __restrict__ d1, float* __restrict__ d2, int nseg) {
  const int64_t total = n * nseg;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / n);
    float* d = k == 0 ? d0 : k == 1 ? d1 : d2;
    d[i - k * n] += src[i];
  }
}

// out = [a; b; c] (n each; c may be null): tgate's concatenated bias
__global__ void cat3_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                            int64_t n, float* __restrict__ out) {
  const int64_t total = n * (c ? 3 : 2);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i / n);
    out[i] = (k == 0 ? a : k == 1 ? b : c)[i - k * n];
  }
}

static unsigned grid_for(int64_t n, int64_t cap = 4096) {
  int64_t g = (n + 255) / 256;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

}  // namespace asrx

using namespace asrx;

extern "C" {

int asrx_ce_fwd1(const float* z, const int64_t* labels, float* loss_r, float* lse, float* loss, float* count,
                 int64_t rows, int64_t V, hipStream_t stream) {
  if (rows == 0) return 0;
  ASRX_REQUIRE(rows < (1LL << 31), "asrx_ce_fwd1: too many rows");
  ce_fwd1_kernel<<<(unsigned)rows, 256, 0, stream>>>(z, labels, loss_r, lse, V);
  ce_reduce_kernel<<<1, 1024, 0, stream>>>(loss_r, labels, rows, loss, count);
  ASRX_LAUNCHED("asrx_ce_fwd1");
}

int asrx_ce_bwd2(const float* z, const int64_t* labels, const float* lse, const float* g, const float* count, float* dz,
                 int64_t rows, int64_t V, hipStream_t stream) {
  if (rows == 0) return 0;
  ce_bwd2_kernel<<<(unsigned)rows, 256, 0, stream>>>(z, labels, lse, g, count, dz, V);
  ASRX_LAUNCHED("asrx_ce_bwd2");
}

int asrx_ce_part_fwd(const float* part, int64_t nparts, const unsigned short* zb, const int64_t* labels, float* loss_r,
                     float* lse, float* loss, float* count, int64_t rows, int64_t V, hipStream_t stream) {
  if (rows == 0) return 0;
  ASRX_REQUIRE(nparts > 0 && rows < (1LL << 33), "asrx_ce_part_fwd: bad shape");
  ce_part_fwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, stream>>>((const float2*)part, (int)nparts, zb, nullptr,
                                                                     labels, loss_r, lse, rows, V);
  ce_reduce_kernel<<<1, 1024, 0, stream>>>(loss_r, labels, rows, loss, count);
  ASRX_LAUNCHED("asrx_ce_part_fwd");
}

int asrx_ce_part_fwd_f32(const float* part, int64_t nparts, const float* zf, const int64_t* labels, float* loss_r,
                         float* lse, float* loss, float* count, int64_t rows, int64_t V, hipStream_t stream) {
  if (rows == 0) return 0;
  ASRX_REQUIRE(nparts > 0 && rows < (1LL << 33), "asrx_ce_part_fwd_f32: bad shape");
  ce_part_fwd_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, stream>>>((const float2*)part, (int)nparts, nullptr, zf,
                                                                     labels, loss_r, lse, rows, V);
  ce_reduce_kernel<<<1, 1024, 0, stream>>>(loss_r, labels, rows, loss, count);
  ASRX_LAUNCHED("asrx_ce_part_fwd_f32");
}

int asrx_head_merge(const float* part, int64_t nparts, const float* zlab, const int64_t* labels, int64_t* pred,
                    float* loss_r, float* lse, float* loss, float* count, int64_t* correct, int64_t rows, int64_t V,
                    hipStream_t stream) {
  if (rows == 0) return 0;
  ASRX_REQUIRE(nparts > 0 && rows < (1LL << 31) && V > 0 && V < (1LL << 31), "asrx_head_merge: bad shape");
  ASRX_REQUIRE(((uintptr_t)part & 7) == 0 && pred, "asrx_head_merge: part 8-byte aligned, pred required");
  ASRX_REQUIRE(!labels || (zlab && loss_r && lse && loss && count && correct),
               "asrx_head_merge: labels need zlab, loss_r, lse, loss, count and correct");
  head_merge_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, stream>>>(
      (const float2*)part, (const int*)(part + 2 * rows * nparts), (int)nparts, zlab, labels, pred, loss_r, lse, rows, V);
  if (labels) {
    ce_reduce_kernel<<<1, 1024, 0, stream>>>(loss_r, labels, rows, loss, count);
    head_count_kernel<<<1, 1024, 0, stream>>>(pred, labels, rows, correct, count);
  }
  ASRX_LAUNCHED("asrx_head_merge");
}

int asrx_ce_bwd_f32in(const float* zf, const int64_t* labels, const float* lse, const float* g, const float* count,
                      unsigned short* dzb, int64_t rows, int64_t V, hipStream_t stream) {
  if (rows == 0) return 0;
  ASRX_REQUIRE(rows < (1LL << 31), "asrx_ce_bwd_f32in: too many rows");
  ce_bwd_f32in_kernel<<<(unsigned)rows, 256, 0, stream>>>(zf, labels, lse, g, count, dzb, V);
  ASRX_LAUNCHED("asrx_ce_bwd_f32in");
}

int asrx_ce_bwd_bf16(const unsigned short* zb, const int64_t* labels, const float* lse, const float* g,
                     const float* count, unsigned short* dzb, int64_t rows, int64_t V, hipStream_t stream) {
  if (rows == 0) return 0;
  ASRX_REQUIRE(rows < (1LL << 31), "asrx_ce_bwd_bf16: too many rows");
  ce_bwd_bf16_kernel<<<(unsigned)rows, 256, 0, stream>>>(zb, labels, lse, g, count, dzb, V);
  ASRX_LAUNCHED("asrx_ce_bwd_bf16");
}

int asrx_bn_running(const float* mean, const float* rstd, float* rm, float* rv, int64_t* nbt, int64_t B, int64_t C,
                    int64_t T, float eps, float momentum, hipStream_t stream) {
  if (C == 0) return 0;
  const float unbias = (float)T / (float)std::max<int64_t>(T - 1, 1);
  bn_running_kernel<<<(unsigned)((C + 255) / 256), 256, 0, stream>>>(mean, rstd, rm, rv, nbt, (int)B, (int)C, eps,
                                                                     unbias, momentum);
  ASRX_LAUNCHED("asrx_bn_running");
}

int asrx_bn_running_lens(const float* mean, const float* rstd, float* rm, float* rv, int64_t* nbt,
                         const int32_t* lens, int64_t B, int64_t C, int64_t T, float eps, float momentum,
                         hipStream_t stream) {
  if (C == 0) return 0;
  ASRX_REQUIRE(lens != nullptr, "asrx_bn_running_lens: per-sample lengths: null table");
  ASRX_REQUIRE(((uintptr_t)lens & 3) == 0, "asrx_bn_running_lens: per-sample lengths: table must be 4-byte aligned");
  bn_running_lens_kernel<<<(unsigned)((C + 255) / 256), 256, 0, stream>>>(mean, rstd, rm, rv, nbt, lens, (int)B,
                                                                          (int)C, (int)T, eps, momentum);
  ASRX_LAUNCHED("asrx_bn_running_lens");
}

int asrx_rsqrt_eps(const float* v, float* out, int64_t n, float eps, hipStream_t stream) {
  if (n == 0) return 0;
  rsqrt_eps_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(v, out, (int)n, eps);
  ASRX_LAUNCHED("asrx_rsqrt_eps");
}

int asrx_conv3_weight(const float* g, const float* v, int64_t Co, int64_t Ci, float* Wt, unsigned short* Wtb, float* Wf,
                      unsigned short* Wfb, float* nrm, hipStream_t stream) {
  if (Co == 0) return 0;
  ASRX_REQUIRE(!g || nrm, "asrx_conv3_weight: weight norm needs nrm");
  conv3_weight_kernel<<<(unsigned)Co, 256, 0, stream>>>(g, v, (int)Co, (int)Ci, Wt, Wtb, Wf, Wfb, nrm);
  ASRX_LAUNCHED("asrx_conv3_weight");
}

int asrx_conv3_weight_bwd(const float* dWt, const float* g, const float* v, const float* nrm, int64_t Co, int64_t Ci,
                          float* dg, float* dv, hipStream_t stream) {
  if (Co == 0) return 0;
  conv3_weight_bwd_kernel<<<(unsigned)Co, 256, 0, stream>>>(dWt, g, v, nrm, (int)Co, (int)Ci, dg, dv);
  ASRX_LAUNCHED("asrx_conv3_weight_bwd");
}

int asrx_blend_fwd(const float* d, const float* g, const float* blend, float* out, int64_t n, hipStream_t stream) {
  ASRX_REQUIRE(n % 4 == 0 && (((uintptr_t)d | (uintptr_t)g | (uintptr_t)out) & 15) == 0,
               "asrx_blend_fwd: 16-byte aligned, n %% 4 == 0 required");
  if (n == 0) return 0;
  blend_fwd_kernel<<<grid_for(n / 4), 256, 0, stream>>>((const float4*)d, (const float4*)g, blend, (float4*)out, n / 4);
  ASRX_LAUNCHED("asrx_blend_fwd");
}

int asrx_blend_bwd(const float* go, const float* d, const float* g, const float* blend, float* dd, float* dg,
                   float* dblend, int64_t n, hipStream_t stream) {
  ASRX_REQUIRE(n % 4 == 0, "asrx_blend_bwd: n %% 4 == 0 required");
  if (n == 0) return 0;
  blend_bwd_kernel<<<grid_for(n / 4, 1024), 256, 0, stream>>>((const float4*)go, (const float4*)d, (const float4*)g,
                                                              blend, (float4*)dd, (float4*)dg, dblend, n / 4);
  ASRX_LAUNCHED("asrx_blend_bwd");
}

int asrx_add_segments(const float* src, int64_t n, float* d0, float* d1, float* d2, int64_t nseg, hipStream_t stream) {
  ASRX_REQUIRE(nseg >= 1 && nseg <= 3, "asrx_add_segments: 1..3 segments");
  if (n == 0) return 0;
  add_segments_kernel<<<grid_for(n * nseg), 256, 0, stream>>>(src, n, d0, d1, d2, (int)nseg);
  ASRX_LAUNCHED("asrx_add_segments");
}

int asrx_cat3(const float* a, const float* b, const float* c, int64_t n, float* out, hipStream_t stream) {
  if (n == 0) return 0;
  cat3_kernel<<<grid_for(n * 3), 256, 0, stream>>>(a, b, c, n, out);
  ASRX_LAUNCHED("asrx_cat3");
}

}  // extern "C"
