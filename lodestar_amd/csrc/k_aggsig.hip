// Per-job aggregate signatures of a same-message package (lb_verify_same_message_batch_agg) and
// grouped signature aggregation (lb_aggregate_signature_groups): the plain sum of the INCLUDED
// decoded signatures of every job, in the 96-byte compressed form a pool stores and a block
// carries (Signature.aggregate(sigs).toBytes(); attestationPool.ts:182-212).  The inputs are
// already in HBM: the signatures k_decode_sigs decoded once for the verification, and per-set
// include flags written on the device from the verdicts (k_sm_include*) or the decode statuses
// (k_inc_status).
// Part of the MI355X BLS verification pipeline; see bls_host.hip for the DAG.
#include "bls_kernels.h"

namespace lb {

#define LB_JS_NONE 0xffffffffu

// Signature.fromBytes(bytes, validate=false) (signatureFromBytesNoCheck): k_decode_sigs without
// the subgroup ladder.
__global__ void __launch_bounds__(TPB, LB_W_DECODE) k_decode_sigs_nocheck(uint32_t n, const uint8_t* __restrict__ sigs,
                                                                          const uint32_t* __restrict__ sig_off,
                                                                          g2j* __restrict__ out_sig,
                                                                          uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = sig_off[i], b = sig_off[i + 1];
  g2a s;
  const uint8_t st = g2_deserialize(s, sigs + a, b - a);
  g2j sj;
  jac_set_inf(sj);
  if (st == LB_ST_OK) jac_from_aff(sj, s);
  out_sig[i] = sj;
  status[i] = st;
}

// Grouped aggregation: a signature is summed when it loaded.
__global__ void __launch_bounds__(256) k_inc_status(uint32_t n, const uint8_t* __restrict__ status,
                                                    uint8_t* __restrict__ inc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inc[i] = status[i] == LB_ST_OK ? 1 : 0;
}

// Include flags after phase 1 of a same-message package: set i of job j is summed when the job
// took the fast path -- the host's rule in sm_advance_launch, from the same four values -- and
// the caller's mask (optional) keeps it.  The sets of every other job start excluded; phase 2's
// verdicts add the valid ones (k_sm_include_retry).
__global__ void __launch_bounds__(256) k_sm_include(uint32_t n_sets, uint32_t n_jobs,
                                                    const uint32_t* __restrict__ job_off,
                                                    const uint8_t* __restrict__ valid, const uint8_t* __restrict__ err,
                                                    const uint8_t* __restrict__ job_bad,
                                                    const uint8_t* __restrict__ job_pkst,
                                                    const uint8_t* __restrict__ mask, uint8_t* __restrict__ inc) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sets) return;
  // the set's job: the first j with job_off[j + 1] > i (empty jobs own no set)
  uint32_t lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (job_off[mid + 1] > i) hi = mid;
    else lo = mid + 1;
  }
  const uint32_t j = lo;
  const bool fast = valid[j] && err[j] == LB_REQ_OK && !job_bad[j] && job_pkst[j] == LB_ST_OK;
  inc[i] = (fast && (!mask || mask[i])) ? 1 : 0;
}

// Include flags after phase 2: retry r is set rset[r], verified alone (the host's rule for
// out_valid in sm_advance_launch).
__global__ void __launch_bounds__(256) k_sm_include_retry(uint32_t n_retry, const uint32_t* __restrict__ rset,
                                                          const uint8_t* __restrict__ rvalid,
                                                          const uint8_t* __restrict__ rerr,
                                                          const uint8_t* __restrict__ mask, uint8_t* __restrict__ inc) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_retry) return;
  const uint32_t i = rset[r];
  inc[i] = (rvalid[r] && rerr[r] == LB_REQ_OK && (!mask || mask[i])) ? 1 : 0;
}

// One wave per workgroup serves jobs_per_wg (<= LB_JS_JOBS) consecutive jobs, grid-stride over
// such runs; the host picks jobs_per_wg so a run holds about one wave of sets (a job of 64 sets
// or more keeps a wave to itself, sixteen 4-set jobs share one).
//   - The run's sets are walked in tiles of 64, lane l taking set base + l.  A lane keeps adding
//     into its register accumulator while its sets stay in one job (a large job: one addition per
//     tile, as k_same_message_agg's strided loop).  When a tile brings a lane a set of another
//     job, the wave flushes: a segmented suffix reduction over the lanes' partials in LDS
//     (log2 64 steps; lane l takes lane l + s while both hold the same job -- jobs are contiguous
//     in lane order), and the first lane of each segment adds its total to the job's LDS record.
//   - Jacobian -> affine for all jobs of the run with ONE Fp2 inversion (Montgomery's trick:
//     prefix products of the non-zero Z on lane 0, one inversion, unwound), then one lane per
//     job: x = X z^-2, y = Y z^-3, g2_compress into out96, the count of summed sets.
// An empty job, or one with nothing included, or whose included signatures cancel, gives the
// compressed infinity encoding (0xc0, 95 zero bytes).
// LDS per workgroup: 64 + 16 LdsRec<g2j> (304 B) + 16 fp2 + 64 + 17 + 16 words, 26,256 B with alignment.
__global__ void __launch_bounds__(TPB) k_job_sig(uint32_t n_jobs, uint32_t jobs_per_wg,
                                                 const uint32_t* __restrict__ job_off, const g2j* __restrict__ sig,
                                                 const uint8_t* __restrict__ inc, uint8_t* __restrict__ out96,
                                                 uint32_t* __restrict__ out_count) {
  __shared__ LdsRec<g2j> sh[TPB];
  __shared__ LdsRec<g2j> jacc[LB_JS_JOBS];
  __shared__ fp2 zpre[LB_JS_JOBS];
  __shared__ uint32_t sjob[TPB];
  __shared__ uint32_t joff[LB_JS_JOBS + 1];
  __shared__ uint32_t cnt[LB_JS_JOBS];
  const uint32_t l = threadIdx.x;
  const uint32_t jpw = jobs_per_wg < 1 ? 1 : jobs_per_wg > LB_JS_JOBS ? LB_JS_JOBS : jobs_per_wg;
  for (uint64_t run = blockIdx.x; run * jpw < n_jobs; run += gridDim.x) {
    const uint32_t j0 = (uint32_t)(run * jpw);
    const uint32_t nw = n_jobs - j0 < jpw ? n_jobs - j0 : jpw;
    if (l <= nw) joff[l] = job_off[j0 + l];
    if (l < nw) {
      g2j z;
      jac_set_inf(z);
      jacc[l].v = z;
      cnt[l] = 0;
    }
    __syncthreads();
    const uint64_t a0 = joff[0], a1 = joff[nw];
    g2j acc;
    jac_set_inf(acc);
    uint32_t accjob = LB_JS_NONE;  // the job (within the run) this lane's partial belongs to
    for (uint64_t base = a0;; base += TPB) {
      const bool last = base >= a1;  // uniform: past the run's sets, only the flush is left
      const uint64_t i = base + l;
      uint32_t jt = LB_JS_NONE;
      if (!last && i < a1) {
        jt = 0;
        while (joff[jt + 1] <= i) jt++;  // (i < a1 = joff[nw]: ends below nw)
      }
      const bool clash = accjob != LB_JS_NONE && jt != LB_JS_NONE && jt != accjob;
      if ((last || __any(clash)) && __any(accjob != LB_JS_NONE)) {
        sh[l].v = acc;
        sjob[l] = accjob;
        __syncthreads();
        for (uint32_t s = 1; s < TPB; s <<= 1) {
          const bool take = accjob != LB_JS_NONE && l + s < TPB && sjob[l + s] == accjob;
          g2j o;
          if (take) o = sh[l + s].v;
          __syncthreads();
          if (take) {
            jac_add(acc, acc, o);
            sh[l].v = acc;
          }
          __syncthreads();
        }
        if (accjob != LB_JS_NONE && (l == 0 || sjob[l - 1] != accjob)) {
          g2j m = jacc[accjob].v;
          jac_add(m, m, acc);
          jacc[accjob].v = m;
        }
        __syncthreads();
        jac_set_inf(acc);
        accjob = LB_JS_NONE;
      }
      if (last) break;
      if (jt != LB_JS_NONE) {
        if (inc[i]) {
          atomicAdd(&cnt[jt], 1u);
          const g2j t = sig[i];
          jac_add(acc, acc, t);
        }
        accjob = jt;
      }
    }
    if (l == 0) {
      fp2 prod;
      fp2_one(prod);
      for (uint32_t g = 0; g < nw; g++) {
        zpre[g] = prod;
        const fp2 z = jacc[g].v.Z;
        if (!fp2_is_zero(z)) fp2_mul(prod, prod, z);
      }
      fp2 inv;
      fp2_inv(inv, prod);  // (a product of non-zero Z, or one)
      for (uint32_t g = nw; g-- > 0;) {
        const fp2 z = jacc[g].v.Z;
        if (fp2_is_zero(z)) continue;
        fp2 zi;
        fp2_mul(zi, inv, zpre[g]);
        fp2_mul(inv, inv, z);
        zpre[g] = zi;
      }
    }
    __syncthreads();
    if (l < nw) {
      const g2j tot = jacc[l].v;
      g2a s;
      if (jac_is_inf(tot)) {
        fp2_zero(s.x);
        fp2_zero(s.y);
        s.inf = true;
      } else {
        const fp2 zi = zpre[l];
        fp2 zi2, zi3;
        fp2_sqr(zi2, zi);
        fp2_mul(zi3, zi2, zi);
        fp2_mul(s.x, tot.X, zi2);
        fp2_mul(s.y, tot.Y, zi3);
        s.inf = false;
      }
      g2_compress(out96 + (size_t)(j0 + l) * 96, s);
      out_count[j0 + l] = cnt[l];
    }
    __syncthreads();
  }
}

}  // namespace lb
