// Randomized same-message aggregation (LB_SM_RANDOMIZED): PK_j = sum s_i pk_i and
// S_j = sum s_i sig_i over job j's sets, s_i = batch_scalar(seed, LB_SM_AGG_INDEX_FLAG | i)
// with i the set's index in the call (blst's aggregateWithRandomness, with the call's DRBG):
// a passing aggregate then implies every set of the job valid except with probability 2^-64,
// where the plain sums of k_same_message_agg accept sig_0 + D, sig_1 - D.  A job of exactly
// one set is not multiplied (the same verdict, no ladder on a single attestation's path).
// The G1 and G2 sides are separate kernels (the host runs them on the slot's two streams);
// they fill the buffers the plain stages fill: d_jpk / d_jpkst / d_pk96, d_sig192 / d_jbad.
// Part of the MI355X BLS verification pipeline; see bls_host.hip for the DAG.
#include "bls_kernels.h"

namespace lb {

// the call's seed in private memory (batch_scalar reads it byte by byte)
LB_DEV uint64_t sm_agg_scalar(const uint8_t* __restrict__ seed, uint32_t i) {
  uint8_t sd[32];
  for (int k = 0; k < 32; k++) sd[k] = seed[k];
  return batch_scalar(sd, LB_SM_AGG_INDEX_FLAG | i);
}

// One wave per job, grid-stride over jobs; lanes take sets a + tid, a + tid + TPB, ...:
// s_i pk_i by the GLV ladder, LDS tree sum, lane 0 writes the job's key (Jacobian + status,
// as k_pubkeys_single / k_pubkeys_agg do, and its 96-byte encoding, as k_same_message_agg does).
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_sm_rand_pk(uint32_t n_jobs, const uint32_t* __restrict__ job_off,
                                                                 PkSource pks, const uint8_t* __restrict__ seed,
                                                                 g1j* __restrict__ out_pk,
                                                                 uint8_t* __restrict__ pk_status,
                                                                 uint8_t* __restrict__ out_pk96) {
  __shared__ LdsRec<g1j> sh[TPB];
  __shared__ uint32_t bad;
  for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
    const uint32_t a = job_off[j], b = job_off[j + 1];
    const bool mul = b - a >= 2;  // uniform across the block
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    g1j acc;
    jac_set_inf(acc);
    for (uint32_t i = a + threadIdx.x; i < b; i += TPB) {
      g1a p;
      const uint8_t st = pk_load(p, pks, i);
      if (st != LB_ST_OK) {
        atomicOr(&bad, 1u);
      } else if (!p.inf) {
        if (mul) {
          g1j t;
          jac_mul_glv_xy(t, p.x, p.y, LB_G1_BETA, LB_G1_BETA2, sm_agg_scalar(seed, i));
          jac_add(acc, acc, t);
        } else {
          jac_from_aff(acc, p);
        }
      }
    }
    sh[threadIdx.x].v = acc;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s && a + threadIdx.x + s < b) {
        g1j o = sh[threadIdx.x + s].v;
        g1j m = sh[threadIdx.x].v;
        jac_add(m, m, o);
        sh[threadIdx.x].v = m;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      g1j tot = sh[0].v;
      out_pk[j] = tot;
      pk_status[j] = a == b ? LB_ST_EMPTY_AGGREGATE : bad ? LB_ST_BAD_ENCODING
                                                   : jac_is_inf(tot) ? LB_ST_PK_INFINITY : LB_ST_OK;
      g1a pa;
      jac_to_aff(pa, tot);
      g1_serialize(out_pk96 + (size_t)j * 96, pa);
    }
    __syncthreads();
  }
}

// The signature side: the job's decoded, validated signatures (k_decode_sigs, once) times
// s_i, summed; the aggregate's 192-byte encoding and job_bad[j] as k_same_message_agg writes
// them (an empty job or one with a signature that failed validation: all zero bytes, bad).
// An infinite decoded signature contributes the identity.
__global__ void __launch_bounds__(TPB, LB_W_SSIG) k_sm_rand_sig(uint32_t n_jobs, const uint32_t* __restrict__ job_off,
                                                                const uint8_t* __restrict__ seed,
                                                                const g2j* __restrict__ sig,
                                                                const uint8_t* __restrict__ sig_status,
                                                                uint8_t* __restrict__ out_sig192,
                                                                uint8_t* __restrict__ job_bad) {
  __shared__ LdsRec<g2j> sh[TPB];
  __shared__ uint32_t bad;
  for (uint32_t j = blockIdx.x; j < n_jobs; j += gridDim.x) {
    const uint32_t a = job_off[j], b = job_off[j + 1];
    const bool mul = b - a >= 2;  // uniform across the block
    if (threadIdx.x == 0) bad = (a == b) ? 1u : 0u;
    __syncthreads();
    g2j acc;
    jac_set_inf(acc);
    for (uint32_t i = a + threadIdx.x; i < b; i += TPB) {
      if (sig_status[i] != LB_ST_OK) {
        atomicOr(&bad, 1u);
      } else if (!jac_is_inf(sig[i])) {
        if (mul) {
          // (a decoded signature's Z is 1: the ladder's result is the point itself)
          g2j t;
          jac_mul_glv_xy(t, sig[i].X, sig[i].Y, LB_G2_OMEGA, LB_G2_OMEGA2, sm_agg_scalar(seed, i));
          jac_add(acc, acc, t);
        } else {
          acc = sig[i];
        }
      }
    }
    sh[threadIdx.x].v = acc;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s && a + threadIdx.x + s < b) {
        g2j o = sh[threadIdx.x + s].v;
        g2j m = sh[threadIdx.x].v;
        jac_add(m, m, o);
        sh[threadIdx.x].v = m;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      uint8_t* os = out_sig192 + (size_t)j * 192;
      if (bad) {
        for (int k = 0; k < 192; k++) os[k] = 0;
      } else {
        g2j tot = sh[0].v;
        g2a s;
        jac_to_aff(s, tot);
        g2_serialize(os, s);
      }
      job_bad[j] = bad ? 1 : 0;
    }
    __syncthreads();
  }
}

}  // namespace lb
