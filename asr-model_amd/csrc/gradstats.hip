// Gradient statistics for the seam between backward and the optimizer step (essentials.py:778-821:
// track_grad_norms, the global norm, GradScaler.unscale_'s inf/NaN check, clip_grad_norm_ and the
// skipped step), for every gradient of the model in two launches and without a host sync.
//
// Output, stats[np + 4]:
//   stats[i]     sum of squares of parameter i's unscaled gradient inv_scale * g
//   ctl[0] coef  inv_scale * min(1, max_norm / (total_norm + eps)); inv_scale when max_norm <= 0;
//                0 when found_inf (torch's clip_grad_norm_ rule on the unscaled gradients)
//   ctl[1]       found_inf (0.0 / 1.0): an element with an all-ones exponent, or a total norm that
//                is not finite (a finite 1e30 overflows its square)
//   ctl[2]       total_norm = sqrt(sum_i stats[i])
//   ctl[3]       number of non-finite elements
// with ctl = stats + np; asrx_maxfactor_step_ex reads ctl[0] and ctl[1].
//
// Layout: every gradient is cut into chunks of GS_CHUNK elements; the chunks of all gradients form
// one flat space (item0 = a parameter's first chunk), one wave takes one chunk.  Gradients that are
// views of a flat bucket (asrx.dist.GradSync) are only 4-byte aligned: GS_CHUNK * 4 bytes is a
// multiple of 16, so every chunk of a tensor has the same misalignment; a chunk peels up to 3 scalar
// elements to the next 16-byte boundary, reads float4, and ends with up to 3 scalars.
// K1 writes one partial (sum, non-finite count) per chunk; K2 (one workgroup) sums each parameter's
// partials and then the parameters in a fixed order, in double.  No atomics: two calls on the same
// input give bit-identical stats.
#include "common.h"

namespace asrx {

struct GSParam {
  const float* g;
  int64_t n;
  int64_t item0;  // first chunk of this gradient in the flat chunk space
};

constexpr int GS_CHUNK = 4096;  // elements per chunk (asrx/optim.py GS_CHUNK): 16 float4 per lane
constexpr int GS_MAXP = 4096;   // gradients per call (the chunk-offset table is staged in LDS)

__device__ __forceinline__ void gs_acc(float x, float c, float& s, unsigned& bad) {
  bad += (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
  const float y = c * x;
  s += y * y;
}

// ---- K1: one wave per chunk -> ws[2 * chunk] = sum (c g)^2, ws[2 * chunk + 1] = non-finite count
__global__ __launch_bounds__(256) void gs_chunks_kernel(const GSParam* __restrict__ tab, int np, int64_t nitems,
                                                        float c, float* __restrict__ ws) {
  __shared__ int64_t offs[GS_MAXP];
  for (int k = threadIdx.x; k < np; k += blockDim.x) offs[k] = tab[k].item0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int64_t it = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); it < nitems; it += (int64_t)gridDim.x * 4) {
    int lo = 0, hi = np - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offs[mid] <= it) lo = mid;
      else hi = mid - 1;
    }
    const int64_t start = (it - offs[lo]) * GS_CHUNK;
    const int64_t left = tab[lo].n - start;
    const int len = left < 0 ? 0 : (int)(left < GS_CHUNK ? left : GS_CHUNK);
    const float* q = tab[lo].g + start;
    const int mis = (int)(((uintptr_t)q >> 2) & 3);  // elements past a 16-byte boundary
    const int head = min((4 - mis) & 3, len);
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;  // [tail0, len): up to 3 elements
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    unsigned bad = 0;
    if (lane < head) gs_acc(q[lane], c, s0, bad);
    const float4* q4 = reinterpret_cast<const float4*>(q + head);
#pragma unroll 4
    for (int v = lane; v < nvec; v += 64) {
      const float4 x = q4[v];
      gs_acc(x.x, c, s0, bad);
      gs_acc(x.y, c, s1, bad);
      gs_acc(x.z, c, s2, bad);
      gs_acc(x.w, c, s3, bad);
    }
    if (tail0 + lane < len) gs_acc(q[tail0 + lane], c, s1, bad);
    float s = wave_sum((s0 + s1) + (s2 + s3));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if (lane == 0) {
      ws[2 * it] = s;
      reinterpret_cast<uint32_t*>(ws)[2 * it + 1] = bad;
    }
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- K2: one workgroup of 16 waves.  Wave w sums the chunk partials of parameters w, w + 16, ...
// (lane l takes partials l, l + 64, ..., then the xor tree: a fixed order), wave 0 then sums the
// parameters the same way and writes the control word.
__global__ __launch_bounds__(1024) void gs_reduce_kernel(const GSParam* __restrict__ tab, int np, int64_t nitems,
                                                         float inv_scale, float max_norm, float eps,
                                                         const float* __restrict__ ws, float* __restrict__ stats) {
  __shared__ double tot[GS_MAXP];
  __shared__ double wbad[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double nbad = 0.0;
  for (int i = w; i < np; i += 16) {
    const int64_t c0 = tab[i].item0, c1 = i + 1 < np ? tab[i + 1].item0 : nitems;
    double s = 0.0, b = 0.0;
    for (int64_t k = c0 + lane; k < c1; k += 64) {
      s += (double)ws[2 * k];
      b += (double)reinterpret_cast<const uint32_t*>(ws)[2 * k + 1];
    }
    s = wave_sum_f64(s);
    nbad += wave_sum_f64(b);
    if (lane == 0) {
      stats[i] = (float)s;
      tot[i] = s;
    }
  }
  if (lane == 0) wbad[w] = nbad;
  __syncthreads();
  if (w != 0) return;
  double s = 0.0;
  for (int i = lane; i < np; i += 64) s += tot[i];
  s = wave_sum_f64(s);
  if (lane != 0) return;
  double bad = 0.0;
  for (int k = 0; k < 16; ++k) bad += wbad[k];
  const float total = (float)sqrt(s);
  const bool inf = bad > 0.0 || !isfinite(total);
  float coef = inv_scale;
  if (max_norm > 0.f) coef = inv_scale * fminf(1.f, max_norm / (total + eps));
  float* ctl = stats + np;
  ctl[0] = inf ? 0.f : coef;
  ctl[1] = inf ? 1.f : 0.f;
  ctl[2] = total;
  ctl[3] = (float)bad;
}

}  // namespace asrx

using namespace asrx;

extern "C" int asrx_grad_stats_param_bytes(void) { return (int)sizeof(GSParam); }

// table: device array of np GSParam (asrx/optim.py packs it), nitems = sum ceil(n / GS_CHUNK);
// stats: np + 4 floats; ws: 2 * nitems floats.
extern "C" int asrx_grad_stats(const void* table, int np, int64_t nitems, float inv_scale, float max_norm, float eps,
                               float* stats, float* ws, hipStream_t stream) {
  ASRX_REQUIRE(np > 0, "asrx_grad_stats: no gradients");
  ASRX_REQUIRE(np <= GS_MAXP, "asrx_grad_stats: at most %d gradients per call (got %d); split the call", GS_MAXP, np);
  ASRX_REQUIRE(nitems >= 0, "asrx_grad_stats: bad chunk count %ld", (long)nitems);
  ASRX_REQUIRE(table && stats && (ws || nitems == 0), "asrx_grad_stats: null pointer");
  const GSParam* tab = reinterpret_cast<const GSParam*>(table);
  if (nitems > 0) {
    const unsigned gr = (unsigned)std::min<int64_t>((nitems + 3) / 4, 2048);
    gs_chunks_kernel<<<gr, 256, 0, stream>>>(tab, np, nitems, inv_scale, ws);
  }
  gs_reduce_kernel<<<1, 1024, 0, stream>>>(tab, np, nitems, inv_scale, max_norm, eps, ws, stats);
  ASRX_LAUNCHED("asrx_grad_stats");
}
