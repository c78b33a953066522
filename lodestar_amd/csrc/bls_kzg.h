// Declarations of the blob KZG verification kernels (k_kzg.hip), kept apart from
// bls_kernels.h so that a change here rebuilds k_kzg.hip and bls_host.hip only.
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
}  // namespace lb
