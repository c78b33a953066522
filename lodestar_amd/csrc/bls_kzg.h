// Declarations of the blob KZG kernels (verification: k_kzg.hip; commitments and proofs:
// k_kzg_msm.hip), kept apart from bls_kernels.h so that a change here rebuilds those two
// units and bls_host.hip only.
#pragma once
#include "bls_kernels.h"
#include "bls_fr.h"

namespace lb {

// SHA-256 blocks of compute_challenge's transcript: 16 + 16 + 131072 + 48 bytes, padded
static constexpr uint32_t LB_KZG_FS_BLOCKS = 2050;
static constexpr uint32_t LB_KZG_HASH_TPB = 128;  // k_kzg_hash: the round lane's wave + the expanding wave
static constexpr uint32_t LB_KZG_EVAL_TPB = 256;  // k_kzg_eval: strips of LB_KZG_N / 256 = 16 elements
// ladders of the tail: batch (3n + 1: rho_i pi_i, rho_i z_i pi_i, rho_i C_i, -(sum rho_i y_i) G1)
// or per item (2n: z_i pi_i, -y_i G1)
enum : uint32_t { LB_KZG_BATCH = 0, LB_KZG_EACH = 1 };

// Fixed-base MSM over the Lagrange setup (k_kzg_msm.hip): signed base-256 digits in
// [-127, 128] of a 255-bit scalar, 32 windows (r < 2^255: the top byte is at most 0x73, so
// the top window takes a carry without overflowing), one set of 128 buckets per job, chunks
// of <= 16 entries.  The table T[j][i] = [2^(8j)] L[i] holds every doubling.
static constexpr uint32_t LB_KZG_MSM_WIN = 32;
static constexpr uint32_t LB_KZG_MSM_NB = 128;
static constexpr uint32_t LB_KZG_MSM_T = 16;
static constexpr uint32_t LB_KZG_MSM_ENT = LB_KZG_MSM_WIN * LB_KZG_N;                     // entries of one job
static constexpr uint32_t LB_KZG_MSM_MAXC = LB_KZG_MSM_ENT / LB_KZG_MSM_T + LB_KZG_MSM_NB;  // its chunks, at most
static constexpr uint32_t LB_KZG_MSM_GROUP = 16;    // jobs that share one set of launches (and the workspace)
static constexpr uint32_t LB_KZG_MSM_SCAT_PER = 8;  // k_kzg_msm_scatter: entries per thread
static constexpr uint32_t LB_KZG_MSM_NONE = 0xffffffffu;

// 8 big-endian words (as they lie in a blob) -> raw little-endian limbs
LB_DEV void kzg_raw_from_words(uint32_t* t, const uint32_t* __restrict__ w) {
#pragma unroll
  for (int j = 0; j < 8; j++) t[j] = __builtin_bswap32(w[7 - j]);
}
LB_DEV bool kzg_load_fr(fr& r, const uint32_t* __restrict__ w) {
  uint32_t t[8];
  kzg_raw_from_words(t, w);
  const bool ok = fr_raw_is_canonical(t);
  fr raw;
#pragma unroll
  for (int j = 0; j < 8; j++) raw.l[j] = ok ? t[j] : 0u;
  fr_to_mont(r, raw);
  return ok;
}
// ... and back: canonical big-endian bytes, as 8 words
LB_DEV void kzg_store_fr(uint32_t* __restrict__ w, const fr& a) {
  fr raw;
  fr_from_mont(raw, a);
#pragma unroll
  for (int j = 0; j < 8; j++) w[j] = __builtin_bswap32(raw.l[7 - j]);
}

__global__ void __launch_bounds__(256) k_kzg_roots(fr* __restrict__ roots);
__global__ void __launch_bounds__(TPB) k_kzg_setup_g2(const uint8_t* __restrict__ in96, g2a* __restrict__ neg_tau,
                                                      uint8_t* __restrict__ status);
__global__ void __launch_bounds__(LB_KZG_HASH_TPB) k_kzg_hash(const uint8_t* __restrict__ blobs,
                                                              const uint8_t* __restrict__ com48,
                                                              uint8_t* __restrict__ z32, uint8_t* __restrict__ status);
__global__ void __launch_bounds__(LB_KZG_EVAL_TPB) k_kzg_eval(const uint8_t* __restrict__ blobs,
                                                              const fr* __restrict__ roots,
                                                              const uint8_t* __restrict__ z32,
                                                              uint8_t* __restrict__ y32, uint8_t* __restrict__ status);
__global__ void __launch_bounds__(TPB) k_kzg_decode(uint32_t n, const uint8_t* __restrict__ com48,
                                                    const uint8_t* __restrict__ proofs48, g1j* __restrict__ P,
                                                    uint8_t* __restrict__ pt_status);
__global__ void __launch_bounds__(TPB) k_kzg_rho(uint32_t n, uint32_t mode, const uint8_t* __restrict__ com48,
                                                 const uint8_t* __restrict__ proofs48,
                                                 const uint8_t* __restrict__ z32, const uint8_t* __restrict__ y32,
                                                 const uint8_t* __restrict__ pt_status, uint8_t* __restrict__ status,
                                                 uint8_t* __restrict__ scalars, uint8_t* __restrict__ skip);
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_ladder(uint32_t n, uint32_t mode,
                                                                 const g1j* __restrict__ P,
                                                                 const uint8_t* __restrict__ scalars,
                                                                 const uint8_t* __restrict__ skip,
                                                                 g1j* __restrict__ out);
__global__ void __launch_bounds__(TPB) k_kzg_each_sum(uint32_t n, const g1j* __restrict__ P,
                                                      const g1j* __restrict__ lad, g1j* __restrict__ AB);
__global__ void __launch_bounds__(TPB, LB_W_TAIL) k_kzg_miller(uint32_t m, const g1j* __restrict__ AB,
                                                               const g2a* __restrict__ neg_tau,
                                                               const uint8_t* __restrict__ skip,
                                                               fp12* __restrict__ f);
__global__ void __launch_bounds__(TPB, LB_W_TAIL) k_kzg_final(uint32_t m, uint32_t mode, const fp12* __restrict__ f,
                                                              const uint8_t* __restrict__ status,
                                                              const uint8_t* __restrict__ skip,
                                                              uint8_t* __restrict__ verdict);

// ---- k_kzg_msm.hip ------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_kzg_setup_g1(const uint8_t* __restrict__ in48, g1j* __restrict__ J,
                                                      g1a* __restrict__ T, uint8_t* __restrict__ status);
__global__ void __launch_bounds__(TPB) k_kzg_check_com(uint32_t n, const uint8_t* __restrict__ com48,
                                                       uint8_t* __restrict__ status);
__global__ void __launch_bounds__(LB_KZG_EVAL_TPB) k_kzg_quotient(const uint8_t* __restrict__ blobs,
                                                                  const fr* __restrict__ roots,
                                                                  const uint8_t* __restrict__ z32,
                                                                  const uint8_t* __restrict__ y32,
                                                                  const uint8_t* __restrict__ status,
                                                                  uint8_t* __restrict__ q32);
__global__ void __launch_bounds__(256) k_kzg_msm_digits(const uint8_t* __restrict__ scalars32,
                                                        uint8_t* __restrict__ status, uint8_t bad_code,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ hist);
__global__ void __launch_bounds__(LB_KZG_MSM_NB) k_kzg_msm_scan(const uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ off, uint32_t* __restrict__ coff,
                                                                uint32_t* __restrict__ cursor);
__global__ void __launch_bounds__(256) k_kzg_msm_scatter(const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                         uint32_t* __restrict__ sorted);
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_chunks(const uint32_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ coff,
                                                                     const uint32_t* __restrict__ sorted,
                                                                     const g1a* __restrict__ T, g1j* __restrict__ csum);
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_buckets(const uint32_t* __restrict__ coff,
                                                                      const g1j* __restrict__ csum,
                                                                      g1j* __restrict__ bsum);
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_bits(const g1j* __restrict__ bsum, g1j* __restrict__ G);
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_final(uint32_t n_jobs, const g1j* __restrict__ G,
                                                                    const uint8_t* __restrict__ status,
                                                                    uint8_t* __restrict__ out48);
}  // namespace lb
