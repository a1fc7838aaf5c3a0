// Entry points of the wide GEMM (kernel and design: gemm_wr.h), the bulk weight conversion to
// bf16 and the MSheath row-tile lists.
#include "gemm_wr.h"
#include "gemm_p2.h"
#include "gemm_ws.h"
#include <string>

// Which wide-GEMM kernel runs the plain / residual products that gemm_p2_kernel covers (asrx_set_gemm_variant):
// 1 gemm_p2_kernel (two workgroups per CU) for tile widths 3 and 2, 2 also for width 1 (the 128-column
// tiles: gemm_p2's NJ = 2 tile is 128 x 128), 0 gemm_wr_kernel -- A/B measurements and the tests that compare them;
// + 4: the weight-stationary gemm_ws_kernel first for the launches it takes (ws_ok: K <= 384, >= 32768 rows, the
// shapes where it measured faster).
// + 16: the AbbyNormal router at d = 64 on gemm_wr_kernel instead of router64_kernel (A/B, tests).
// Default 5.
static int g_wide_variant = 5;
extern "C" int asrx_set_gemm_variant(int v) {
  const int old = g_wide_variant;
  g_wide_variant = v;
  return old;
}

// The kernel of a plain, residual or rotary product (asrx_gemm_wn_ex, _res, _rot): gemm_ws where it is on and
// takes the launch, else gemm_p2 where it does, else gemm_wr.  Every choice computes the same bits, so only a
// profile shows a change here.
enum class WideKernel { WS, P2, WR };
static WideKernel wide_kernel(const asrx::wn::Params& p, asrx::wn::Epi epi, int conv, int nj, int a_bf16) {
  const int v = g_wide_variant;
  // + 4: gemm_ws on; + 8: at every shape it can run (tests), not only those where it measured faster (ws_ok)
  if ((v & 4) != 0 && !conv && asrx::wn::ws_ok(p, a_bf16, (v & 8) != 0)) return WideKernel::WS;
  // gemm_p2_kernel takes: no k3 conv, float4-aligned C / Z (LDS-staged epilogue), tile widths 3 and 2 -- for the
  // residual and rotary epilogues 3 only, the one width they are instantiated at
  // (measured, profiles/r05_p2_micro.txt: bf16-stored A 5-10 % faster at every shape; fp32 A faster up to 96000
  // rows but 9-18 % slower at 192064 rows, where its four A loads per thread and k-step cost more than the
  // overlap gains -- so fp32 A at >= 131072 rows stays on gemm_wr_kernel)
  const bool vec = ((p.N | p.ldc) & 3) == 0 && ((uintptr_t)p.C & 15) == 0 && ((uintptr_t)p.Z & 15) == 0 &&
                   ((uintptr_t)p.Cb & 7) == 0;
  const bool width = epi == asrx::wn::Epi::Plain ? nj == 3 || nj == 2 || (nj == 1 && (v & 3) == 2) : nj == 3;
  if ((a_bf16 || p.M < 131072) && (v & 3) >= 1 && !conv && width && vec && p.K >= 64) return WideKernel::P2;
  return WideKernel::WR;
}

namespace asrx {
namespace wn {

// fp32 (rows x cols, row stride ld) -> bf16 N x K contiguous.  trans == 0: N = rows, K = cols;
// trans == 1: N = cols, K = rows (the weight is used transposed, e.g. dgrad's dY W).
__global__ void weight_to_bf16_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int rows,
                                      int cols, int64_t ld, int trans) {
  const int64_t total = (int64_t)rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r, c, o;
    if (!trans) {
      r = i / cols;
      c = i % cols;
      o = r * cols + c;
    } else {
      c = i / rows;  // output row n = source column
      r = i % rows;
      o = c * rows + r;
    }
    __bf16 h = (__bf16)src[r * ld + c];
    dst[o] = __builtin_bit_cast(unsigned short, h);
  }
}

}  // namespace wn
}  // namespace asrx

using namespace asrx;

extern "C" int asrx_weight_to_bf16(const float* src, unsigned short* dst, int64_t rows, int64_t cols, int64_t ld,
                                   int trans, hipStream_t stream) {
  if (rows * cols == 0) return 0;
  const int64_t n = rows * cols;
  wn::weight_to_bf16_kernel<<<(unsigned)std::min<int64_t>((n + 255) / 256, 16384), 256, 0, stream>>>(
      src, dst, (int)rows, (int)cols, ld, trans);
  ASRX_LAUNCHED("asrx_weight_to_bf16");
}

// Every GEMM weight of a step converted in ONE launch (asrx/gemm.py bulk plan): entry e converts
// src (rows x cols, row stride ld) to bf16 dst (N x K contiguous; trans as weight_to_bf16).  A
// workgroup walks one entry's elements; grid (ceil(max elements / 4096), entries).
struct WConv {
  const float* src;
  unsigned short* dst;
  int64_t ld;
  int rows, cols, trans, pad;
};

namespace asrx {
__global__ __launch_bounds__(256) void weights_to_bf16_kernel(const WConv* __restrict__ tab) {
  const WConv e = tab[blockIdx.y];
  const int64_t total = (int64_t)e.rows * e.cols;
  const int64_t i0 = (int64_t)blockIdx.x * 4096;
  if (i0 >= total) return;
  const int64_t i1 = min<int64_t>(total, i0 + 4096);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    int64_t r, c, o;
    if (!e.trans) {
      r = i / e.cols;
      c = i % e.cols;
      o = r * e.cols + c;
    } else {
      c = i / e.rows;
      r = i % e.rows;
      o = c * e.rows + r;
    }
    e.dst[o] = __builtin_bit_cast(unsigned short, (__bf16)e.src[r * e.ld + c]);
  }
}
}  // namespace asrx

extern "C" int64_t asrx_wconv_entry_bytes(void) { return (int64_t)sizeof(WConv); }

// tab: n device-resident WConv entries (asrx_wconv_entry_bytes() each); max_elems: the largest
// rows * cols among them.
extern "C" int asrx_weights_to_bf16(const void* tab, int64_t n, int64_t max_elems, hipStream_t stream) {
  if (n == 0) return 0;
  ASRX_REQUIRE(n < 65536, "asrx_weights_to_bf16: too many entries");
  dim3 grid((unsigned)((max_elems + 4095) / 4096), (unsigned)n);
  weights_to_bf16_kernel<<<grid, 256, 0, stream>>>((const WConv*)tab);
  ASRX_LAUNCHED("asrx_weights_to_bf16");
}

// What the wide-GEMM entry points below share.
//
// wide_check: the four checks each of them makes, in this order -- a non-empty problem, A and W 16-byte aligned,
// K and the row strides divisible, operands that span < 2^31 elements.  An entry point extends the second and
// third with conditions of its own (Also: their value, and its wording of the whole check) and may name a failure
// of its own that is reported right after the first check (early) or right before the last (late).  0, or 2 with
// the message set.
struct Also { bool ok; const char* msg; };
static int wide_check(const char* name, const void* A, int a_bf16, int64_t lda, const void* W, int64_t ldw, int64_t M,
                      int64_t N, int64_t K, Also aligned = {true, "A/W must be 16-byte aligned"},
                      Also strides = {true, "K%8, lda%4, ldw%8 required"}, const char* early = nullptr,
                      const char* late = nullptr) {
  ASRX_REQUIRE(M > 0 && N > 0 && K > 0, "%s: empty problem", name);
  ASRX_REQUIRE(!early, "%s: %s", name, early);
  ASRX_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0 && aligned.ok, "%s: %s", name, aligned.msg);
  ASRX_REQUIRE(K % 8 == 0 && lda % (a_bf16 ? 8 : 4) == 0 && ldw % 8 == 0 && strides.ok, "%s: %s", name, strides.msg);
  ASRX_REQUIRE(!late, "%s: %s", name, late);
  ASRX_REQUIRE(M * lda < (1LL << 31) && N * ldw < (1LL << 31), "%s: operand spans >= 2^31 elements", name);
  return 0;
}

// wide_params: the operands every product has; every other field is null / 0 (convF = convC = 1: no conv) and is
// assigned by name where an entry point uses it.
static wn::Params wide_params(const void* A, int64_t lda, const unsigned short* W, int64_t ldw, float* C, int64_t ldc,
                              const float* bias, float* Z, int64_t M, int64_t N, int64_t K, float alpha = 1.f,
                              float beta = 0.f, int act = ACT_NONE) {
  wn::Params p{};
  p.A = (const float*)A; p.lda = (int)lda; p.W = W; p.ldw = (int)ldw;
  p.C = C; p.ldc = (int)ldc; p.bias = bias; p.Z = Z;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.convF = p.convC = 1;
  p.alpha = alpha; p.beta = beta; p.act = act;
  return p;
}

// run_wr / run_wide: runtime tile width (3, 2, otherwise 1), conv and A storage -> the template instance.  Only
// instances that exist are named (wr_built / p2_built / ws_built beside the lists in gemm_wr.h, gemm_p2.h,
// gemm_ws.h): naming another would compile a second copy of the kernel into this unit.  false: no instance
// (launched() reports it; the entry points' own checks leave no such call).
template <wn::Epi EPI, int NJ, bool CONV, bool ABF>
static bool wr_instance(const wn::Params& p, hipStream_t s) {
  if constexpr (wn::wr_built(NJ, CONV, ABF, EPI)) wn::launch_wr<NJ, CONV, ABF, EPI>(p, s);
  return wn::wr_built(NJ, CONV, ABF, EPI);
}
template <wn::Epi EPI, int NJ, bool ABF>
static bool p2_instance(const wn::Params& p, hipStream_t s) {
  if constexpr (wn::p2_built(NJ, ABF, EPI)) wn::launch_p2_act<NJ, ABF, EPI>(p, s);
  return wn::p2_built(NJ, ABF, EPI);
}
template <wn::Epi EPI, bool ABF>
static bool ws_instance(const wn::Params& p, hipStream_t s) {
  if constexpr (wn::ws_built(ABF, EPI)) wn::launch_ws_act<ABF, EPI>(p, s);
  return wn::ws_built(ABF, EPI);
}
template <wn::Epi EPI, int NJ>
static bool run_wr_nj(const wn::Params& p, int conv, int a_bf16, hipStream_t s) {
  if (conv) return a_bf16 ? wr_instance<EPI, NJ, wn::CONV3, wn::BF16A>(p, s) : wr_instance<EPI, NJ, wn::CONV3, wn::F32A>(p, s);
  return a_bf16 ? wr_instance<EPI, NJ, wn::ROWS, wn::BF16A>(p, s) : wr_instance<EPI, NJ, wn::ROWS, wn::F32A>(p, s);
}
template <wn::Epi EPI>  // gemm_wr_kernel only
static bool run_wr(const wn::Params& p, int conv, int nj, int a_bf16, hipStream_t s) {
  return nj == 3 ? run_wr_nj<EPI, 3>(p, conv, a_bf16, s)
                 : nj == 2 ? run_wr_nj<EPI, 2>(p, conv, a_bf16, s) : run_wr_nj<EPI, 1>(p, conv, a_bf16, s);
}
template <wn::Epi EPI>  // the kernel wide_kernel chooses; gemm_p2 runs widths 2 and 1 on its 128 x 128 (NJ = 2) tile
static bool run_wide(const wn::Params& p, int conv, int nj, int a_bf16, hipStream_t s) {
  switch (wide_kernel(p, EPI, conv, nj, a_bf16)) {
    case WideKernel::WS: return a_bf16 ? ws_instance<EPI, wn::BF16A>(p, s) : ws_instance<EPI, wn::F32A>(p, s);
    case WideKernel::P2:
      if (nj == 3) return a_bf16 ? p2_instance<EPI, 3, wn::BF16A>(p, s) : p2_instance<EPI, 3, wn::F32A>(p, s);
      return a_bf16 ? p2_instance<EPI, 2, wn::BF16A>(p, s) : p2_instance<EPI, 2, wn::F32A>(p, s);
    default: return run_wr<EPI>(p, conv, nj, a_bf16, s);
  }
}
static int launched(bool ran, const char* name) {
  ASRX_REQUIRE(ran, "%s: no kernel instance for this call", name);
  return check_launch(name);
}

// Y (M x N, ldc) = act(alpha * A W^T + beta * Y + bias); A fp32 (M x K, lda) or its k3 im2col
// (conv: lda = channels, K = 3 * channels, segment length convF); W bf16 (N x K, ldw).  nj selects
// the tile width 128 * nj (1..3).
extern "C" int asrx_gemm_wn(const float* A, int64_t lda, int conv, int64_t convF, int64_t convC,
                            const unsigned short* W, int64_t ldw, float* C, int64_t ldc, const float* bias, float* Z,
                            int64_t M, int64_t N, int64_t K, float alpha, float beta, int act, int nj,
                            hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn", A, 0, lda, W, ldw, M, N, K)) return rc;
  ASRX_REQUIRE(!conv || (convF > 0 && convC % 4 == 0), "asrx_gemm_wn: conv needs F > 0 and C %% 4 == 0");
  wn::Params p = wide_params(A, lda, W, ldw, C, ldc, bias, Z, M, N, K, alpha, beta, act);
  p.convF = (int)(convF > 0 ? convF : 1);
  p.convC = (int)(convC > 0 ? convC : 1);
  return launched(run_wr<wn::Epi::Plain>(p, conv, nj, 0, stream), "asrx_gemm_wn");
}

// asrx_gemm_wn with storage types: A fp32 (a_bf16 = 0) or bf16 (1); C fp32 (c_bf16 = 0) or bf16 (1,
// beta = 0; Z, when given, stays fp32); optionally restricted to the device tile list mtiles (as
// asrx_gemm_wn_rows, non-conv only).
extern "C" int asrx_gemm_wn_ex(const void* A, int a_bf16, int64_t lda, int conv, int64_t convF, int64_t convC,
                               const unsigned short* W, int64_t ldw, void* C, int c_bf16, int64_t ldc,
                               const float* bias, float* Z, int64_t M, int64_t N, int64_t K, float alpha, float beta,
                               int act, int nj, const int* mtiles, const int* n_mtiles, hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn_ex", A, a_bf16, lda, W, ldw, M, N, K, {true, "A/W must be 16-byte aligned"},
                          {true, "K%8, lda%4 (fp32) / lda%8 (bf16), ldw%8 required"}))
    return rc;
  ASRX_REQUIRE(!conv || (convF > 0 && convC % (a_bf16 ? 8 : 4) == 0), "asrx_gemm_wn_ex: conv needs F > 0 and C %% 4 (8 for bf16)");
  ASRX_REQUIRE(!c_bf16 || beta == 0.f, "asrx_gemm_wn_ex: a bf16 output takes beta = 0");
  ASRX_REQUIRE(!(conv && mtiles), "asrx_gemm_wn_ex: tile lists are for plain GEMMs");
  wn::Params p = wide_params(A, lda, W, ldw, c_bf16 ? nullptr : (float*)C, ldc, bias, Z, M, N, K, alpha, beta, act);
  p.convF = (int)(convF > 0 ? convF : 1);
  p.convC = (int)(convC > 0 ? convC : 1);
  p.mtiles = mtiles;
  p.n_mtiles = n_mtiles;
  p.Cb = c_bf16 ? (unsigned short*)C : nullptr;
  return launched(run_wide<wn::Epi::Plain>(p, conv, nj, a_bf16, stream), "asrx_gemm_wn_ex");
}

// Tied logits with the cross entropy's statistics fused (model.py:629 logits = x @ token.weight^T,
// model.py:670 F.cross_entropy): Zb (M x N, ldc) = bf16(A W^T) for a bf16-stored A, and per row and
// 128*nj-column tile the (max, sum exp(z - max)) of the tile's bf16 logits in part[row * nparts + tile]
// (float2, nparts = ceil(N / (128 nj))) -- asrx_ce_part_fwd turns them into the loss without re-reading
// the logits.
extern "C" int asrx_gemm_wn_ce(const void* A, int64_t lda, const unsigned short* W, int64_t ldw, unsigned short* Zb,
                               int64_t ldc, float* part, int64_t M, int64_t N, int64_t K, int nj, hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn_ce", A, 1, lda, W, ldw, M, N, K,
                          {((uintptr_t)Zb & 7) == 0 && ((uintptr_t)part & 7) == 0, "A/W 16-byte, Zb/part 8-byte aligned"},
                          {N % 4 == 0 && ldc % 4 == 0, "K, lda, ldw % 8 and N, ldc % 4 required"}))
    return rc;
  ASRX_REQUIRE(nj >= 1 && nj <= 3, "asrx_gemm_wn_ce: nj in 1..3");
  wn::Params p = wide_params(A, lda, W, ldw, nullptr, ldc, nullptr, nullptr, M, N, K);
  p.Cb = Zb;
  p.ce_part = (float2*)part;
  p.ce_ld = (int)((N + 128 * nj - 1) / (128 * nj));
  return launched(run_wr<wn::Epi::CE>(p, 0, nj, 1, stream), "asrx_gemm_wn_ce");
}

// As asrx_gemm_wn_ce with the logits stored fp32 (Zf) and the statistics taken of the fp32 values.
extern "C" int asrx_gemm_wn_ce_f32(const void* A, int64_t lda, const unsigned short* W, int64_t ldw, float* Zf,
                               int64_t ldc, float* part, int64_t M, int64_t N, int64_t K, int nj, hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn_ce_f32", A, 1, lda, W, ldw, M, N, K,
                          {((uintptr_t)Zf & 15) == 0 && ((uintptr_t)part & 7) == 0,
                           "A/W 16-byte, Zf 16-byte, part 8-byte aligned"},
                          {N % 4 == 0 && ldc % 4 == 0, "K, lda, ldw % 8 and N, ldc % 4 required"}))
    return rc;
  ASRX_REQUIRE(nj >= 1 && nj <= 3, "asrx_gemm_wn_ce_f32: nj in 1..3");
  wn::Params p = wide_params(A, lda, W, ldw, Zf, ldc, nullptr, nullptr, M, N, K);
  p.ce_part = (float2*)part;
  p.ce_ld = (int)((N + 128 * nj - 1) / (128 * nj));
  return launched(run_wr<wn::Epi::CE>(p, 0, nj, 1, stream), "asrx_gemm_wn_ce_f32");
}

// Logits-free head (essentials.py:875-935 evaluation: model(...)["loss"] and torch.argmax(logits, -1);
// model.py:691-699 the greedy step's argmax): the tied-logits product of asrx_gemm_wn_ce_f32 without the
// logits store.  part: M x nparts float2 (max, sum exp(z - max)) of each 128*nj-column tile's fp32 logits --
// the numbers asrx_gemm_wn_ce_f32 writes -- followed by M x nparts int32, the column of that max (the lowest
// among equal maxima; INT_MAX for a tile without a value above -inf).  labels (nullable, int64 per row): the
// logit of each row's label goes to zlab[row]; label 0 and labels outside [0, N) write nothing.  lda may
// exceed K (the last position of each sample through a strided view).  asrx_head_merge finishes the rows.
extern "C" int asrx_gemm_wn_head(const void* A, int64_t lda, const unsigned short* W, int64_t ldw, float* part,
                                 const int64_t* labels, float* zlab, int64_t M, int64_t N, int64_t K, int nj,
                                 hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn_head", A, 1, lda, W, ldw, M, N, K,
                          {((uintptr_t)part & 7) == 0, "A/W 16-byte, part 8-byte aligned"},
                          {N % 4 == 0 && lda >= K, "K, lda, ldw % 8, N % 4 and lda >= K required"}))
    return rc;
  ASRX_REQUIRE(nj >= 1 && nj <= 3, "asrx_gemm_wn_head: nj in 1..3");
  ASRX_REQUIRE(!labels || zlab, "asrx_gemm_wn_head: labels need zlab");
  const int64_t nparts = (N + 128 * nj - 1) / (128 * nj);
  wn::Params p = wide_params(A, lda, W, ldw, nullptr, N, nullptr, nullptr, M, N, K);
  p.ce_part = (float2*)part;
  p.ce_ld = (int)nparts;
  p.hd_idx = reinterpret_cast<int*>(part + 2 * M * nparts);
  p.hd_labels = labels;
  p.hd_zlab = zlab;
  return launched(run_wr<wn::Epi::Head>(p, 0, nj, 1, stream), "asrx_gemm_wn_head");
}

// Out projection with its residual add (model.py:578-580 x = x + attn(...).out): C = R + A W^T + bias, A, C
// and R fp32 (R may not alias C), 16-byte aligned rows; nj 1 or 3 (the residual epilogue is compiled into
// dedicated instantiations only, so the other GEMMs keep their register budget).
extern "C" int asrx_gemm_wn_res(const float* A, int64_t lda, const unsigned short* W, int64_t ldw, float* C, int64_t ldc,
                                const float* bias, const float* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int nj,
                                hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn_res", A, 0, lda, W, ldw, M, N, K,
                          {((uintptr_t)C & 15) == 0 && ((uintptr_t)R & 15) == 0, "A/W/C/R must be 16-byte aligned"},
                          {N % 4 == 0 && ldc % 4 == 0 && ldr % 4 == 0, "K, ldw % 8; lda, N, ldc, ldr % 4"}))
    return rc;
  ASRX_REQUIRE(R && R != C, "asrx_gemm_wn_res: a residual input distinct from C is required");
  ASRX_REQUIRE(nj == 1 || nj == 3, "asrx_gemm_wn_res: nj 1 or 3");
  wn::Params p = wide_params(A, lda, W, ldw, C, ldc, bias, nullptr, M, N, K);
  p.Rres = R;
  p.ldr = (int)ldr;
  return launched(run_wide<wn::Epi::Res>(p, 0, nj, 0, stream), "asrx_gemm_wn_res");
}

// q / k projection with rotary fused (model.py:242-245 then 198-214, with the hd^-0.25 scale of model.py:303-304):
// C = rot(A W^T + bias), i.e. each head's pairs (2j, 2j+1) of the product times polar(scale * m[row], angle(row %
// L, j)) from the (cos, sin) table tab (positions >= L, hd / 2) float2 -- asrx_rotary_fwd2's arithmetic, so C is
// bit-identical to the GEMM followed by that pass; Z (nullable) receives the unrotated product (what the rotary
// backward reads).  A fp32 (a_bf16 = 0) or bf16 (1); C, Z fp32, 16-byte aligned rows; nj 1 or 3.
extern "C" int asrx_gemm_wn_rot(const void* A, int a_bf16, int64_t lda, const unsigned short* W, int64_t ldw,
                                float* C, float* Z, int64_t ldc, const float* bias, const float* m, const float* tab,
                                int64_t L, int64_t hd, float scale, int64_t M, int64_t N, int64_t K, int nj,
                                hipStream_t stream) {
  const bool heads = hd >= 4 && hd % 4 == 0 && N % hd == 0;
  if (int rc = wide_check("asrx_gemm_wn_rot", A, a_bf16, lda, W, ldw, M, N, K,
                          {((uintptr_t)C & 15) == 0 && ((uintptr_t)Z & 15) == 0 && ((uintptr_t)tab & 15) == 0,
                           "A/W/C/Z/tab must be 16-byte aligned"},
                          {N % 4 == 0 && ldc % 4 == 0, "K, ldw % 8; lda % 4 (8 bf16); N, ldc % 4"},
                          L > 0 ? nullptr : "empty problem", heads ? nullptr : "head dim % 4, N % hd"))
    return rc;
  ASRX_REQUIRE(m && tab, "asrx_gemm_wn_rot: row norms and angle table required");
  ASRX_REQUIRE(nj == 1 || nj == 3, "asrx_gemm_wn_rot: nj 1 or 3");
  wn::Params p = wide_params(A, lda, W, ldw, C, ldc, bias, Z, M, N, K);
  p.rot_m = m;
  p.rot_tab = reinterpret_cast<const float2*>(tab);
  p.rot_L = (int)L;
  p.rot_half = (int)(hd / 2);
  p.rot_scale = scale;
  return launched(run_wide<wn::Epi::Rot>(p, 0, nj, a_bf16, stream), "asrx_gemm_wn_rot");
}

// Backward of y = act(A W^T + bias) (act gelu / silu / sigmoid) without a stored pre-activation: the GEMM
// recomputes z = A W^T + bias with the forward's tile width (nj 3 only: the instantiation the forward's
// shapes use) and writes gz = bf16(G * act'(z)) (M x N, ldc) from the output gradient G (fp32, ldg), adding
// the column sums of gz into db when non-null.  A fp32 (a_bf16 = 0) or bf16 (1).
extern "C" int asrx_gemm_wn_gact(const void* A, int a_bf16, int64_t lda, const unsigned short* W, int64_t ldw,
                                 const float* bias, const float* G, int64_t ldg, unsigned short* gz, int64_t ldc,
                                 float* db, int64_t M, int64_t N, int64_t K, int act, int nj, hipStream_t stream) {
  const char* early = nj != 3 ? "nj 3 only"
                      : act != ACT_GELU && act != ACT_SILU && act != ACT_SIGMOID ? "gelu/silu/sigmoid only" : nullptr;
  if (int rc = wide_check("asrx_gemm_wn_gact", A, a_bf16, lda, W, ldw, M, N, K,
                          {((uintptr_t)G & 15) == 0 && ((uintptr_t)gz & 7) == 0, "A/W/G 16-byte, gz 8-byte aligned"},
                          {N % 4 == 0 && ldc % 4 == 0 && ldg % 4 == 0, "K, ldw % 8; lda % 4 (8 bf16); N, ldc, ldg % 4"},
                          early))
    return rc;
  wn::Params p = wide_params(A, lda, W, ldw, nullptr, ldc, bias, nullptr, M, N, K, 1.f, 0.f, act);
  p.Cb = gz;
  p.G = G;
  p.ldg = (int)ldg;
  p.dB = db;
  return launched(run_wr<wn::Epi::GAct>(p, 0, nj, a_bf16, stream), "asrx_gemm_wn_gact");
}

// asrx_gemm_wn restricted to the BM-row tiles listed in mtiles (n_mtiles entries, both on the device,
// from asrx_row_tiles); rows of other tiles are not written.
extern "C" int asrx_gemm_wn_rows(const float* A, int64_t lda, const unsigned short* W, int64_t ldw, float* C,
                                 int64_t ldc, const float* bias, float* Z, int64_t M, int64_t N, int64_t K,
                                 float alpha, float beta, int act, int nj, const int* mtiles, const int* n_mtiles,
                                 hipStream_t stream) {
  if (int rc = wide_check("asrx_gemm_wn_rows", A, 0, lda, W, ldw, M, N, K)) return rc;
  ASRX_REQUIRE(mtiles && n_mtiles, "asrx_gemm_wn_rows: tile list required");
  wn::Params p = wide_params(A, lda, W, ldw, C, ldc, bias, Z, M, N, K, alpha, beta, act);
  p.mtiles = mtiles;
  p.n_mtiles = n_mtiles;
  return launched(run_wr<wn::Epi::Plain>(p, 0, nj, 0, stream), "asrx_gemm_wn_rows");
}

// The BM-row tiles of an M-row activation whose rows r belong to a sample b = r / L that is at MSheath
// layer `layer` (next_i[b] == layer): mtiles[0 .. *n_mtiles) in increasing order.  One workgroup.
// LENS (asrx_row_lens_tiles; next_i may be null: every sample at the layer): a tile is listed only if it holds a live
// row, l < T_b = lens[b] clamped to [0, L], of a sample at the layer -- all-pad tiles are skipped like inactive samples.
namespace asrx {
template <bool LENS = false>
__global__ __launch_bounds__(1024) void row_tiles_kernel(const float* __restrict__ next_i, int layer, int64_t L,
                                                         int64_t M, int* __restrict__ mtiles, int* __restrict__ n_out,
                                                         const int32_t* __restrict__ lens = nullptr) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int nm = (int)((M + wn::BM - 1) / wn::BM);
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int t0 = 0; t0 < nm; t0 += 1024) {
    const int t = t0 + threadIdx.x;
    int act = 0;
    if (t < nm) {
      const int64_t r0 = (int64_t)t * wn::BM, r1 = min<int64_t>(r0 + wn::BM, M) - 1;
      if constexpr (LENS) {
        for (int64_t b = r0 / L; b <= r1 / L && !act; ++b) {
          const int64_t Tb = min<int64_t>(max(lens[b], 0), L);
          // the sample's live rows [b L, b L + T_b) meet the tile's [r0, r1]
          act = (!next_i || next_i[b] == (float)layer) && b * L + Tb > r0 && b * L <= r1 && Tb > 0;
        }
      } else {
        for (int64_t b = r0 / L; b <= r1 / L && !act; ++b) act = next_i[b] == (float)layer;
      }
    }
    // block exclusive scan of act
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int v = act;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o);
      if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int off = base;
    for (int k = 0; k < w; ++k) off += wsum[k];
    if (act) mtiles[off + v - 1] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
      for (int k = 0; k < 16; ++k) tot += wsum[k];
      base += tot;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) n_out[0] = base;
}
}  // namespace asrx

extern "C" int64_t asrx_row_tiles_max(int64_t M) { return (M + wn::BM - 1) / wn::BM; }

extern "C" int asrx_row_tiles(const float* next_i, int64_t layer, int64_t L, int64_t M, int* mtiles, int* n_mtiles,
                              hipStream_t stream) {
  ASRX_REQUIRE(L > 0 && M > 0, "asrx_row_tiles: empty");
  row_tiles_kernel<false><<<1, 1024, 0, stream>>>(next_i, (int)layer, L, M, mtiles, n_mtiles);
  ASRX_LAUNCHED("asrx_row_tiles");
}

extern "C" int asrx_row_lens_tiles(const float* next_i, int64_t layer, const int32_t* lens, int64_t L, int64_t M,
                                   int* mtiles, int* n_mtiles, hipStream_t stream) {
  ASRX_REQUIRE(L > 0 && M > 0, "asrx_row_tiles: empty");
  ASRX_REQUIRE(lens != nullptr, "asrx_row_lens_tiles: per-sample lengths: null table");
  ASRX_REQUIRE(((uintptr_t)lens & 3) == 0, "asrx_row_lens_tiles: per-sample lengths: table must be 4-byte aligned");
  row_tiles_kernel<true><<<1, 1024, 0, stream>>>(next_i, (int)layer, L, M, mtiles, n_mtiles, lens);
  ASRX_LAUNCHED("asrx_row_lens_tiles");
}

// AbbyNormal router (essentials.py:155-161) in one pass: h_pre = A W1^T + b1 (kept in hpre when
// non-null, for the backward) and logits = SiLU(h_pre) W2^T (M x 3, without b2), for d <= 384.
namespace asrx {
namespace wn {

// AbbyNormal router at d = 64 (the per-head norms of model.py:303-304's q / k; essentials.py:155-161):
// logits = SiLU(x W1^T + b1) W2^T over 1.15 M rows of 64 features at the tiny config.  gemm_wr_kernel ran it on
// a 128-column tile with half the columns empty and two k-steps per 128-row tile (prologue and epilogue bound,
// 1.8 TB/s).  Here a wave streams 16-row groups straight from global memory into MFMA fragments: W1 (64 x 64 bf16)
// sits in 32 registers as the row operand for the whole launch, each group is 8 v_mfma_f32_16x16x32_bf16, and the
// epilogue reduces in registers.  The fragment layout, k order, epilogue expressions and the logit sum order
// (each 32-column group over its lane's columns, xor-16 / xor-32 partners, then the groups in order, plus the
// two empty groups' +0.0) are gemm_wr_kernel's (epilogue_router), so h_pre and the logits are bit-identical.
// The next group's x is in flight while a group is computed (two named register sets, loop unrolled by two).
struct R64X {
  float4 v[4];  // lane (row l & 15): k 8 (l >> 4) .. + 7 of k-halves 0 and 1
};
__global__ __launch_bounds__(256) void router64_kernel(Params p) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  bf16x8 wf[4][2];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
      wf[nb][kb] = *reinterpret_cast<const bf16x8*>(p.W + (int64_t)(16 * nb + lr) * p.ldw + 32 * kb + 8 * lk);
  float bv[4][4], w2v[3][4][4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = 16 * nb + 4 * lk + q;
      bv[nb][q] = p.bias ? p.bias[n] : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) w2v[k][nb][q] = p.W2[k * 64 + n];
    }
  const int64_t ngroups = ((int64_t)p.M + 15) / 16;
  const int64_t step = (int64_t)gridDim.x * 4;
  const float* A = reinterpret_cast<const float*>(p.A);
  auto fetch = [&](int64_t g, R64X& x) __attribute__((always_inline)) {
    const int64_t row = min(g * 16 + lr, (int64_t)p.M - 1);  // past the end: a valid row, results dropped
    const float* src = A + row * p.lda + 8 * lk;
    x.v[0] = *reinterpret_cast<const float4*>(src);
    x.v[1] = *reinterpret_cast<const float4*>(src + 4);
    x.v[2] = *reinterpret_cast<const float4*>(src + 32);
    x.v[3] = *reinterpret_cast<const float4*>(src + 36);
  };
  auto group = [&](int64_t g, const R64X& x) __attribute__((always_inline)) {
    bf16x8 xf[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const float4 a = x.v[2 * kb], b = x.v[2 * kb + 1];
      xf[kb] = bf16x8{(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w,
                      (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
    }
    f32x4 acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb][kb], xf[kb], acc[nb], 0, 0, 0);
    const int64_t row = g * 16 + lr;
    float s[2][3];
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int nb = 2 * grp + nt;
        const float v[4] = {p.alpha * acc[nb][0] + bv[nb][0], p.alpha * acc[nb][1] + bv[nb][1],
                            p.alpha * acc[nb][2] + bv[nb][2], p.alpha * acc[nb][3] + bv[nb][3]};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float h = silu_f(v[q]);
          s0 += h * w2v[0][nb][q];
          s1 += h * w2v[1][nb][q];
          s2 += h * w2v[2][nb][q];
        }
        if (p.C && row < p.M)
          *reinterpret_cast<float4*>(p.C + row * p.ldc + 16 * nb + 4 * lk) = make_float4(v[0], v[1], v[2], v[3]);
      }
      s0 += __shfl_xor(s0, 16); s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
      s0 += __shfl_xor(s0, 32); s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
      s[grp][0] = s0; s[grp][1] = s1; s[grp][2] = s2;
    }
    if (lk == 0 && row < p.M) {
#pragma unroll
      for (int k = 0; k < 3; ++k) p.R[row * 3 + k] = s[0][k] + s[1][k] + 0.f + 0.f;
    }
  };
  int64_t g = (int64_t)blockIdx.x * 4 + wid;
  if (g >= ngroups) return;
  R64X xa, xb;
  fetch(g, xa);
  fetch(g + step, xb);
  for (;; g += 2 * step) {
    {
      const R64X x = xa;
      fetch(g + 2 * step, xa);
      group(g, x);
    }
    if (g + step >= ngroups) break;
    {
      const R64X x = xb;
      fetch(g + 3 * step, xb);
      group(g + step, x);
    }
    if (g + 2 * step >= ngroups) break;
  }
}

}  // namespace wn
}  // namespace asrx

extern "C" int asrx_gemm_wn_router(const float* A, int64_t lda, const unsigned short* W1, int64_t ldw,
                                   const float* b1, const float* W2, float* hpre, int64_t ldc, float* logits,
                                   int64_t M, int64_t N, int64_t K, hipStream_t stream) {
  ASRX_REQUIRE(M > 0 && N > 0 && K > 0, "asrx_gemm_wn_router: empty problem");
  ASRX_REQUIRE(N <= 384, "asrx_gemm_wn_router: N must be <= 384 (one tile column)");
  ASRX_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W1 & 15) == 0, "asrx_gemm_wn_router: A/W must be 16-byte aligned");
  ASRX_REQUIRE(K % 8 == 0 && lda % 4 == 0 && ldw % 8 == 0, "asrx_gemm_wn_router: K%%8, lda%%4, ldw%%8 required");
  ASRX_REQUIRE(M * lda < (1LL << 31), "asrx_gemm_wn_router: operand spans >= 2^31 elements");
  wn::Params p = wide_params(A, lda, W1, ldw, hpre, ldc, b1, nullptr, M, N, K);
  p.W2 = W2;
  p.R = logits;
  const bool r64 = N == 64 && K == 64 && W2 && (g_wide_variant & 16) == 0 && ldw % 8 == 0 &&
                   (!hpre || (ldc % 4 == 0 && ((uintptr_t)hpre & 15) == 0));
  if (r64) {
    static int cus = 0;
    if (!cus) {
      int dev = 0;
      (void)hipGetDevice(&dev);
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
      cus = std::max(1, cus);
    }
    const int64_t groups = (M + 15) / 16;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((groups + 3) / 4, (int64_t)cus * 8));
    wn::router64_kernel<<<grid, 256, 0, stream>>>(p);
    ASRX_LAUNCHED("asrx_gemm_wn_router");
  }
  return launched(run_wr<wn::Epi::Router>(p, 0, N <= 128 ? 1 : N <= 256 ? 2 : 3, 0, stream), "asrx_gemm_wn_router");
}
