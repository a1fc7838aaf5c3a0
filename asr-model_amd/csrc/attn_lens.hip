// Attention with per-sample query and key lengths: the entry points asrx_lattn_fwd / asrx_lattn_bwd.
//
// `lens` is a device table of B x 2 int32, {q_len, k_len} per sample, read by the LENS instantiations of the
// attention kernels (attn.hip: exact fp32, attn_mf.hip: bf16 MFMA).  Sample b's query rows [0, q_len) attend
// to its keys [0, k_len) exactly as a B = 1 call with Lq = q_len, Lk = k_len does (same tiles from row 0, same
// order of sums).  Rows past a length are dead: O, lse and dQ rows >= q_len and dK, dV rows >= k_len are stored
// as zeros, and no live result depends on what q / k / v / dO hold there.  The kernels clamp each length to
// [0, Lq] / [0, Lk]; workgroups with no live row store their zeros and return.  Lq and Lk remain the launch
// extents: grid, tensor addressing, the lse rows and the delta_ws workspace (B*H*Lq floats; unspecified on dead
// rows) are those of the uniform call.
//
// The argument checks are those of asrx_attn_fwd2 / asrx_attn_bwd2 (attn.hip), in the same order and words,
// plus three: fp8 is refused (after the precision check), and `lens` must be non-null and 4-byte aligned
// (after the tensor alignment check).  Every check answers before anything is launched, the Delta pass
// included.
#include "common.h"

namespace asrx {
int attn_fwd_mf_lens(int io, const void* q, const int64_t* sq, const void* k, const int64_t* sk, const void* v,
                     const int64_t* sv, void* o, const int64_t* so, float* lse, const int32_t* lens, int64_t B,
                     int64_t H, int64_t Lq, int64_t Lk, int64_t hd, int causal, float scale, hipStream_t stream);
int attn_bwd_mf_lens(int io, const void* q, const int64_t* sq, const void* k, const int64_t* sk, const void* v,
                     const int64_t* sv, const void* dO, const int64_t* sd, const float* lse, const float* delta,
                     float* dq, const int64_t* sdq, float* dk, const int64_t* sdk, float* dv, const int64_t* sdv,
                     const int32_t* lens, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t hd, int causal,
                     float scale, hipStream_t stream);
void attn_fwd_f32_lens(const float* q, const int64_t* sq, const float* k, const int64_t* sk, const float* v,
                       const int64_t* sv, float* o, const int64_t* so, float* lse, const int32_t* lens, int64_t B,
                       int64_t H, int64_t Lq, int64_t Lk, int64_t hd, int causal, float scale, hipStream_t stream);
void attn_bwd_f32_lens(const float* q, const int64_t* sq, const float* k, const int64_t* sk, const float* v,
                       const int64_t* sv, const float* dO, const int64_t* sd, const float* lse, const float* delta,
                       float* dq, const int64_t* sdq, float* dk, const int64_t* sdk, float* dv, const int64_t* sdv,
                       const int32_t* lens, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t hd, int causal,
                       float scale, hipStream_t stream);
void attn_delta(int prec, int io, const void* o, const int64_t* so, const void* dO, const int64_t* sd,
                float* delta_ws, int64_t B, int64_t H, int64_t Lq, int64_t hd, hipStream_t stream);
constexpr int PREC_FP8ATT = 2;
}  // namespace asrx

using namespace asrx;

static bool attn_ok(const int64_t* st) { return st[0] % 4 == 0 && st[1] % 4 == 0 && st[2] % 4 == 0; }
static bool attn_ok8(const int64_t* st) { return st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0; }

extern "C" int asrx_lattn_fwd(int prec, int io, const void* q_, const int64_t* sq, const void* k_, const int64_t* sk,
                              const void* v_, const int64_t* sv, void* o_, const int64_t* so, float* lse,
                              const int32_t* lens, int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t hd,
                              int causal, float scale, hipStream_t stream) {
  const float *q = (const float*)q_, *k = (const float*)k_, *v = (const float*)v_;
  float* o = (float*)o_;
  ASRX_REQUIRE(io == 0 || prec == PREC_BF16, "attention: bf16 storage (io %d) is a bf16-mode layout", io);
  ASRX_REQUIRE(hd == 64 || hd == 128, "attention: head dim %ld unsupported (64 or 128)", (long)hd);
  ASRX_REQUIRE(attn_ok(sq) && attn_ok(sk) && attn_ok(sv) && attn_ok(so), "attention: strides must be multiples of 4");
  ASRX_REQUIRE(!(io & 1) || (attn_ok8(sq) && attn_ok8(sk) && attn_ok8(sv)),
               "attention: strides of bf16-stored operands must be multiples of 8");
  ASRX_REQUIRE(H < 65536 && B < 65536, "attention: grid too large");
  if (B * H * Lq == 0) return 0;
  ASRX_REQUIRE(Lk > 0, "attention: empty key sequence");
  const bool al16 = (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0;
  ASRX_REQUIRE(prec == PREC_F32 || prec == PREC_BF16 || prec == PREC_FP8ATT, "attention: bad precision %d", prec);
  ASRX_REQUIRE(prec != PREC_FP8ATT, "attention: per-sample lengths are not built for the fp8 forward");
  ASRX_REQUIRE(prec == PREC_F32 || al16, "attention: bf16/fp8 modes need 16-byte aligned q/k/v/o");
  ASRX_REQUIRE(lens != nullptr, "attention: per-sample lengths: null table");
  ASRX_REQUIRE(((uintptr_t)lens & 3) == 0, "attention: per-sample lengths: table must be 4-byte aligned");
  if (prec == PREC_BF16)
    attn_fwd_mf_lens(io, q, sq, k, sk, v, sv, o, so, lse, lens, B, H, Lq, Lk, hd, causal, scale, stream);
  else
    attn_fwd_f32_lens(q, sq, k, sk, v, sv, o, so, lse, lens, B, H, Lq, Lk, hd, causal, scale, stream);
  ASRX_LAUNCHED("asrx_lattn_fwd");
}

// delta_ws: workspace of B*H*Lq floats.
extern "C" int asrx_lattn_bwd(int prec, int io, const void* q_, const int64_t* sq, const void* k_, const int64_t* sk,
                              const void* v_, const int64_t* sv, const void* o_, const int64_t* so, const void* dO_,
                              const int64_t* sd, const float* lse, float* delta_ws, float* dq, const int64_t* sdq,
                              float* dk, const int64_t* sdk, float* dv, const int64_t* sdv, const int32_t* lens,
                              int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t hd, int causal, float scale,
                              hipStream_t stream) {
  const float *q = (const float*)q_, *k = (const float*)k_, *v = (const float*)v_;
  const float* dO = (const float*)dO_;
  ASRX_REQUIRE(io == 0 || prec == PREC_BF16, "attention backward: bf16 storage (io %d) is a bf16-mode layout", io);
  ASRX_REQUIRE(prec == PREC_F32 || prec == PREC_BF16, "attention backward: precision %d (fp8 is forward only)", prec);
  ASRX_REQUIRE(hd == 64 || hd == 128, "attention: head dim %ld unsupported (64 or 128)", (long)hd);
  ASRX_REQUIRE(attn_ok(sq) && attn_ok(sk) && attn_ok(sv) && attn_ok(so) && attn_ok(sd) && attn_ok(sdq) &&
                   attn_ok(sdk) && attn_ok(sdv),
               "attention: strides must be multiples of 4");
  ASRX_REQUIRE((!(io & 1) || (attn_ok8(sq) && attn_ok8(sk) && attn_ok8(sv))) && (!(io & 4) || attn_ok8(sd)),
               "attention: strides of bf16-stored operands must be multiples of 8");
  ASRX_REQUIRE(H < 65536 && B < 65536, "attention: grid too large");
  if (B * H * Lq == 0) return 0;
  ASRX_REQUIRE(Lk > 0, "attention: empty key sequence");
  // every check stands ahead of the first launch (Delta): a rejected call has launched nothing
  const bool al16 = (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dO | (uintptr_t)dq | (uintptr_t)dk |
                       (uintptr_t)dv) & 15) == 0;
  ASRX_REQUIRE(prec == PREC_F32 || al16, "attention backward: bf16 mode needs 16-byte aligned tensors");
  ASRX_REQUIRE(lens != nullptr, "attention: per-sample lengths: null table");
  ASRX_REQUIRE(((uintptr_t)lens & 3) == 0, "attention: per-sample lengths: table must be 4-byte aligned");
  attn_delta(prec, io, o_, so, dO_, sd, delta_ws, B, H, Lq, hd, stream);
  if (prec == PREC_BF16)
    attn_bwd_mf_lens(io, q, sq, k, sk, v, sv, dO, sd, lse, delta_ws, dq, sdq, dk, sdk, dv, sdv, lens, B, H, Lq, Lk, hd,
                     causal, scale, stream);
  else
    attn_bwd_f32_lens(q, sq, k, sk, v, sv, dO, sd, lse, delta_ws, dq, sdq, dk, sdk, dv, sdv, lens, B, H, Lq, Lk, hd,
                      causal, scale, stream);
  ASRX_LAUNCHED("asrx_lattn_bwd");
}
