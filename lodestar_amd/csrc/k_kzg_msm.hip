// Blob KZG commitments and proofs (deneb blob_to_kzg_commitment, compute_blob_kzg_proof,
// compute_kzg_proof): the quotient polynomial over Fr and a fixed-base MSM over the
// Lagrange G1 setup.
//
// Reference: ckzg.blobToKzgCommitment / computeBlobKzgProof (packages/beacon-node/src/util/
// kzg.ts:15-22; callers execution/engine/mock.ts:317-318, test/unit/util/kzg.test.ts);
// semantics after consensus-specs deneb polynomial-commitments.md.
//
// One job is sum_i s_i L[i] over the 4096 setup points, s_i < r.  The base is fixed, so the
// table T[j][i] = [2^(8j)] L[i] (32 x 4096 affine points, built once per setup) holds every
// doubling: with signed base-256 digits d_ij in [-127, 128] of s_i,
//   sum_i s_i L[i] = sum_(b = 1..128) b B_b,   B_b = sum_(|d_ij| = b) sign(d_ij) T[j][i]
// which is at most 131,072 mixed additions into ONE set of 128 buckets, and no doubling.
//
//   k_kzg_setup_g1     lane / setup point : validate_kzg_g1, 248 doublings, one inversion
//   k_kzg_check_com    lane / commitment  : bytes_to_kzg_commitment of compute_blob_kzg_proof
//   k_kzg_quotient     workgroup / blob   : q_i = (f_i - y) / (w_i - z), and the in-domain q_m
//   k_kzg_msm_digits   lane / scalar      : canonical test, the 32 digits, bucket histogram
//   k_kzg_msm_scan     workgroup / job    : bucket and chunk offsets (prefix sums)
//   k_kzg_msm_scatter  8 entries / lane   : counting-sort placement
//   k_kzg_msm_chunks   lane / chunk of <= 16 entries of ONE bucket: mixed additions
//   k_kzg_msm_buckets  wave / bucket      : sum of its chunk partials
//   k_kzg_msm_bits     wave / bit k       : G_k = sum of the buckets b with bit k set
//   k_kzg_msm_final    lane / job         : sum_k 2^k G_k (Horner, 7 doublings), 48 bytes
// The jobs of a call share the launches: the job is blockIdx.y, every per-job array is at
// job x its size.  Organisation and hazards as k_msm.hip: buckets are
// written by plain stores of whole points, the only atomics count entries.
#include "bls_kzg.h"

namespace lb {

static_assert(LB_KZG_MSM_ENT % (256 * LB_KZG_MSM_SCAT_PER) == 0, "scatter blocks tile a job's entries");
static_assert(LB_KZG_N % 256 == 0, "digit blocks tile a job's scalars");

// ---- setup ------------------------------------------------------------------
// Lane i (spec order) takes line brp(i) of the file: L[i] = file[brp(i)].  status[] is in file
// order (LB_ST_*).  T[j][i] = [2^(8j)] L[i], affine: the lane walks its 248 doublings
// once, parking the Jacobian points in J and the running product of their Z in T[j][i].x,
// inverts the last product, and walks back (Montgomery's trick: 1 / Z_j = inv x the product
// before it).  A refused point fills its column with infinity; the host drops the table.
__global__ void __launch_bounds__(TPB) k_kzg_setup_g1(const uint8_t* __restrict__ in48, g1j* __restrict__ J,
                                                      g1a* __restrict__ T, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= LB_KZG_N) return;
  const uint32_t fi = __brev(i) >> 20;  // 12-bit reversal
  g1j p;
  {
    g1a a;
    uint8_t st = g1_deserialize(a, in48 + (size_t)fi * 48, 48);
    if (st == LB_ST_OK) {
      jac_from_aff(p, a);
      if (!g1_in_subgroup(p)) st = LB_ST_NOT_IN_GROUP;
    }
    if (st != LB_ST_OK) jac_set_inf(p);
    status[fi] = st;
  }
  fp one, run;
  fp_one(one);
  run = one;
#pragma unroll 1
  for (uint32_t j = 0; j < LB_KZG_MSM_WIN; j++) {
    if (j > 0) {
#pragma unroll 1
      for (int k = 0; k < 8; k++) jac_dbl(p, p);
    }
    const size_t at = (size_t)j * LB_KZG_N + i;
    J[at] = p;
    fp z = p.Z;
    if (fp_is_zero(z)) z = one;
    fp_mul(run, run, z);
    T[at].x = run;
  }
  fp inv;
  fp_inv(inv, run);
#pragma unroll 1
  for (int j = (int)LB_KZG_MSM_WIN - 1; j >= 0; j--) {
    const size_t at = (size_t)j * LB_KZG_N + i;
    const g1j q = J[at];
    const bool inf = jac_is_inf(q);
    fp zi = inv;
    if (j > 0) {
      const fp pre = T[at - LB_KZG_N].x;
      fp_mul(zi, inv, pre);
    }
    fp z = q.Z;
    if (inf) z = one;
    fp_mul(inv, inv, z);
    g1a a;
    fp zi2, zi3;
    fp_sqr(zi2, zi);
    fp_mul(zi3, zi2, zi);
    fp_mul(a.x, q.X, zi2);
    fp_mul(a.y, q.Y, zi3);
    a.inf = inf;
    if (inf) {
      fp_zero(a.x);
      fp_zero(a.y);
    }
    T[at] = a;
  }
}

// bytes_to_kzg_commitment: a status already set stays (the blob is read first)
__global__ void __launch_bounds__(TPB) k_kzg_check_com(uint32_t n, const uint8_t* __restrict__ com48,
                                                       uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1a a;
  uint8_t st = g1_deserialize(a, com48 + (size_t)i * 48, 48);
  if (st == LB_ST_OK) {
    g1j j;
    jac_from_aff(j, a);
    if (!g1_in_subgroup(j)) st = LB_ST_NOT_IN_GROUP;
  }
  if (st != LB_ST_OK && status[i] == LB_KZG_OK) status[i] = LB_KZG_BAD_COMMITMENT;
}

// ---- quotient -----------------------------------------------------------------
// compute_kzg_proof_impl's quotient in evaluation form, q32: 4096 x 32 canonical big-endian
// bytes (what k_kzg_msm_digits reads, like a blob).  z and y are k_kzg_eval's bytes; an item
// with a status gets q = 0.
//   q_i = (f_i - y) / (w_i - z)                                            (w_i != z)
//   q_m = sum_(i != m) (f_i - y) w_i / (z (z - w_i)) = -(1 / z) sum_(i != m) q_i w_i   (z = w_m)
// Strips and inversions as k_kzg_eval: thread t owns elements t, t + 256, ..., one Fr
// inversion per thread over its 16 differences, the zero difference at i = m replaced by 1.
__global__ void __launch_bounds__(LB_KZG_EVAL_TPB) k_kzg_quotient(const uint8_t* __restrict__ blobs,
                                                                  const fr* __restrict__ roots,
                                                                  const uint8_t* __restrict__ z32,
                                                                  const uint8_t* __restrict__ y32,
                                                                  const uint8_t* __restrict__ status,
                                                                  uint8_t* __restrict__ q32) {
  constexpr int STRIP = LB_KZG_N / LB_KZG_EVAL_TPB;
  __shared__ fr sh[LB_KZG_EVAL_TPB];
  __shared__ uint32_t s_eq;
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* blob_w = reinterpret_cast<const uint32_t*>(blobs + (size_t)b * LB_KZG_BLOB_BYTES);
  uint32_t* q_w = reinterpret_cast<uint32_t*>(q32 + (size_t)b * LB_KZG_BLOB_BYTES);
  if (status[b] != LB_KZG_OK) {  // (uniform over the workgroup)
    for (uint32_t k = tid; k < LB_KZG_BLOB_BYTES / 4; k += LB_KZG_EVAL_TPB) q_w[k] = 0;
    return;
  }
  if (tid == 0) s_eq = 0xffffffffu;
  __syncthreads();
  fr z, y, one;
  kzg_load_fr(z, reinterpret_cast<const uint32_t*>(z32 + (size_t)b * 32));
  kzg_load_fr(y, reinterpret_cast<const uint32_t*>(y32 + (size_t)b * 32));
  fr_one(one);
  fr pre[STRIP];
  fr run = one;
#pragma unroll
  for (int k = 0; k < STRIP; k++) {
    const uint32_t i = tid + (uint32_t)k * LB_KZG_EVAL_TPB;
    const fr w = roots[i];
    fr d;
    fr_sub(d, w, z);
    if (fr_is_zero(d)) {
      s_eq = i;  // (the roots are distinct: at most one writer)
      d = one;
    }
    fr_mul(run, run, d);
    pre[k] = run;
  }
  fr inv;
  fr_inv(inv, run);
  __syncthreads();
  const uint32_t m = s_eq;
  fr sum;
  fr_zero(sum);
#pragma unroll
  for (int k = STRIP - 1; k >= 0; k--) {
    const uint32_t i = tid + (uint32_t)k * LB_KZG_EVAL_TPB;
    const fr w = roots[i];
    fr d, ik, f, q;
    fr_sub(d, w, z);
    if (fr_is_zero(d)) d = one;
    if (k > 0)
      fr_mul(ik, inv, pre[k > 0 ? k - 1 : 0]);
    else
      ik = inv;
    fr_mul(inv, inv, d);
    kzg_load_fr(f, blob_w + 8 * i);
    fr_sub(f, f, y);
    fr_mul(q, f, ik);
    if (i != m) {
      kzg_store_fr(q_w + 8 * i, q);
      if (m != 0xffffffffu) {
        fr t;
        fr_mul(t, q, w);
        fr_add(sum, sum, t);
      }
    }
  }
  if (m == 0xffffffffu) return;  // (uniform)
  sh[tid] = sum;
  __syncthreads();
  for (uint32_t s = LB_KZG_EVAL_TPB / 2; s > 0; s >>= 1) {
    if (tid < s) {
      fr a = sh[tid], o = sh[tid + s];
      fr_add(a, a, o);
      sh[tid] = a;
    }
    __syncthreads();
  }
  if (tid == 0) {
    fr zi, q;
    fr_inv(zi, z);  // (z is a root of unity: not zero)
    fr_mul(q, sh[0], zi);
    fr_neg(q, q);
    kzg_store_fr(q_w + 8 * m, q);
  }
}

// ---- the MSM ------------------------------------------------------------------
// Lane (job, i): scalar i of the job, 32 big-endian bytes.  A scalar >= r marks the job
// (status[job] = bad_code unless a status is set already) and counts as 0, so no digit
// leaves [-127, 128].  keys[job][j 4096 + i] = bucket (|d| - 1) with the sign in bit 31, or
// LB_KZG_MSM_NONE for d = 0: the entry's index is its table index.  The histogram is summed
// in LDS first: one global atomic per bucket and workgroup.
__global__ void __launch_bounds__(256) k_kzg_msm_digits(const uint8_t* __restrict__ scalars32,
                                                        uint8_t* __restrict__ status, uint8_t bad_code,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[LB_KZG_MSM_NB];
  __shared__ uint32_t s_bad;
  const uint32_t job = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * 256 + tid;  // i < LB_KZG_N (grid)
  if (tid < LB_KZG_MSM_NB) s_h[tid] = 0;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  uint32_t t[8];
  kzg_raw_from_words(t, reinterpret_cast<const uint32_t*>(scalars32 + ((size_t)job * LB_KZG_N + i) * 32));
  const bool ok = fr_raw_is_canonical(t);
  if (!ok) {
    s_bad = 1;
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = 0;
  }
  uint32_t* kj = keys + (size_t)job * LB_KZG_MSM_ENT + i;
  uint32_t carry = 0;
#pragma unroll
  for (uint32_t j = 0; j < LB_KZG_MSM_WIN; j++) {
    const uint32_t raw = ((t[j >> 2] >> (8 * (j & 3))) & 0xffu) + carry;
    const bool neg = raw > LB_KZG_MSM_NB;  // never in the top window: its byte is at most 0x73
    const uint32_t mag = neg ? 256u - raw : raw;
    carry = neg ? 1u : 0u;
    kj[(size_t)j * LB_KZG_N] = mag == 0 ? LB_KZG_MSM_NONE : (mag - 1u) | (neg ? 0x80000000u : 0u);
    if (mag != 0) atomicAdd(&s_h[mag - 1u], 1u);
  }
  __syncthreads();
  if (tid < LB_KZG_MSM_NB && s_h[tid]) atomicAdd(&hist[job * LB_KZG_MSM_NB + tid], s_h[tid]);
  if (tid == 0 && s_bad && status[job] == LB_KZG_OK) status[job] = bad_code;
}

// One workgroup per job, one lane per bucket: exclusive prefix sums of the entries (off) and
// of the chunks of <= LB_KZG_MSM_T entries (coff), the totals at [LB_KZG_MSM_NB]; zeroes the
// scatter cursors.
__global__ void __launch_bounds__(LB_KZG_MSM_NB) k_kzg_msm_scan(const uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ off, uint32_t* __restrict__ coff,
                                                                uint32_t* __restrict__ cursor) {
  __shared__ uint32_t se[LB_KZG_MSM_NB], sc[LB_KZG_MSM_NB];
  const uint32_t job = blockIdx.x, t = threadIdx.x;
  const uint32_t h = hist[job * LB_KZG_MSM_NB + t], c = (h + LB_KZG_MSM_T - 1) / LB_KZG_MSM_T;
  se[t] = h;
  sc[t] = c;
  cursor[job * LB_KZG_MSM_NB + t] = 0;
  __syncthreads();
  for (uint32_t s = 1; s < LB_KZG_MSM_NB; s <<= 1) {  // Hillis-Steele, inclusive
    const uint32_t ve = t >= s ? se[t - s] : 0u, vc = t >= s ? sc[t - s] : 0u;
    __syncthreads();
    se[t] += ve;
    sc[t] += vc;
    __syncthreads();
  }
  uint32_t* o = off + job * (LB_KZG_MSM_NB + 1);
  uint32_t* co = coff + job * (LB_KZG_MSM_NB + 1);
  o[t] = se[t] - h;
  co[t] = sc[t] - c;
  if (t == LB_KZG_MSM_NB - 1) {
    o[LB_KZG_MSM_NB] = se[t];
    co[LB_KZG_MSM_NB] = sc[t];
  }
}

// Counting-sort placement: sorted[job][pos] = table index | sign, grouped by bucket.  A
// workgroup ranks its 2,048 entries per bucket in LDS, reserves each bucket's run with one
// global atomic, then stores.  (The order inside a bucket follows the atomics; the bucket's
// sum is the same group element either way.)
__global__ void __launch_bounds__(256) k_kzg_msm_scatter(const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                         uint32_t* __restrict__ sorted) {
  __shared__ uint32_t s_cnt[LB_KZG_MSM_NB], s_base[LB_KZG_MSM_NB];
  const uint32_t job = blockIdx.y, tid = threadIdx.x;
  const uint32_t e0 = blockIdx.x * (256 * LB_KZG_MSM_SCAT_PER) + tid;  // + 256 k < LB_KZG_MSM_ENT (grid)
  if (tid < LB_KZG_MSM_NB) s_cnt[tid] = 0;
  __syncthreads();
  const uint32_t* kj = keys + (size_t)job * LB_KZG_MSM_ENT;
  uint32_t key[LB_KZG_MSM_SCAT_PER], rank[LB_KZG_MSM_SCAT_PER];
#pragma unroll
  for (uint32_t k = 0; k < LB_KZG_MSM_SCAT_PER; k++) {
    key[k] = kj[e0 + 256 * k];
    rank[k] = key[k] == LB_KZG_MSM_NONE ? 0u : atomicAdd(&s_cnt[key[k] & 0x7fffffffu], 1u);
  }
  __syncthreads();
  if (tid < LB_KZG_MSM_NB)
    s_base[tid] = off[job * (LB_KZG_MSM_NB + 1) + tid] +
                  (s_cnt[tid] ? atomicAdd(&cursor[job * LB_KZG_MSM_NB + tid], s_cnt[tid]) : 0u);
  __syncthreads();
  uint32_t* sj = sorted + (size_t)job * LB_KZG_MSM_ENT;
#pragma unroll
  for (uint32_t k = 0; k < LB_KZG_MSM_SCAT_PER; k++) {
    if (key[k] == LB_KZG_MSM_NONE) continue;
    // (s_base + rank < off[bucket + 1] <= LB_KZG_MSM_ENT: the histogram counted this entry)
    sj[s_base[key[k] & 0x7fffffffu] + rank[k]] = (e0 + 256 * k) | (key[k] & 0x80000000u);
  }
}

// table point of a sorted entry, negated by the sign bit
LB_DEV void kzg_msm_point(g1a& q, const g1a* __restrict__ T, uint32_t v) {
  q = T[v & 0x7fffffffu];
  if (v >> 31) fp_neg(q.y, q.y);
}

// One lane per chunk: the sum of <= LB_KZG_MSM_T table points of one bucket, by mixed
// additions.  Both exceptional branches of jac_add_aff are reachable: two setup points may be
// equal or opposite, and T[j + 1][i] = [256] T[j][i] meets T[j][k] when L[k] = [256] L[i].
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_chunks(const uint32_t* __restrict__ off,
                                                                     const uint32_t* __restrict__ coff,
                                                                     const uint32_t* __restrict__ sorted,
                                                                     const g1a* __restrict__ T, g1j* __restrict__ csum) {
  const uint32_t job = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t* o = off + job * (LB_KZG_MSM_NB + 1);
  const uint32_t* co = coff + job * (LB_KZG_MSM_NB + 1);
  if (c >= LB_KZG_MSM_MAXC || c >= co[LB_KZG_MSM_NB]) return;
  uint32_t lo = 0, hi = LB_KZG_MSM_NB;  // the last bucket with coff <= c: the non-empty one holding c
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (co[mid] <= c)
      lo = mid;
    else
      hi = mid;
  }
  const uint32_t e0 = o[lo] + (c - co[lo]) * LB_KZG_MSM_T;
  const uint32_t e1 = min(e0 + LB_KZG_MSM_T, o[lo + 1]);
  const uint32_t* sj = sorted + (size_t)job * LB_KZG_MSM_ENT;
  g1a q;
  kzg_msm_point(q, T, sj[e0]);
  g1j acc;
  jac_from_aff(acc, q);
#pragma unroll 1
  for (uint32_t e = e0 + 1; e < e1; e++) {
    kzg_msm_point(q, T, sj[e]);
    jac_add_aff(acc, acc, q);
  }
  csum[(size_t)job * LB_KZG_MSM_MAXC + c] = acc;
}

// sum of a wave's points: lanes' values through an LDS tree, the total in sh[0]
LB_DEV void kzg_wave_sum(LdsRec<g1j>* sh, const g1j& acc) {
  sh[threadIdx.x].v = acc;
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = TPB / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      g1j m = sh[threadIdx.x].v, o = sh[threadIdx.x + s].v;
      jac_add(m, m, o);
      sh[threadIdx.x].v = m;
    }
    __syncthreads();
  }
}

// One wave per bucket: B_b = sum of its chunk partials (a full job has ~64 per bucket:
// one per lane), infinity when empty
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_buckets(const uint32_t* __restrict__ coff,
                                                                      const g1j* __restrict__ csum,
                                                                      g1j* __restrict__ bsum) {
  __shared__ LdsRec<g1j> sh[TPB];
  const uint32_t job = blockIdx.y, bk = blockIdx.x;  // bk < LB_KZG_MSM_NB (grid)
  const uint32_t* co = coff + job * (LB_KZG_MSM_NB + 1);
  const g1j* cs = csum + (size_t)job * LB_KZG_MSM_MAXC;
  const uint32_t c0 = co[bk], c1 = co[bk + 1];
  g1j acc;
  jac_set_inf(acc);
#pragma unroll 1
  for (uint32_t c = c0 + threadIdx.x; c < c1; c += TPB) {
    const g1j v = cs[c];
    jac_add(acc, acc, v);
  }
  kzg_wave_sum(sh, acc);
  if (threadIdx.x == 0) bsum[job * LB_KZG_MSM_NB + bk] = sh[0].v;
}

// One wave per bit k of the bucket number b = 1..128: G_k = sum of the B_b with bit k set
// (64 of them for k < 7, b = 128 alone for k = 7)
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_bits(const g1j* __restrict__ bsum, g1j* __restrict__ G) {
  __shared__ LdsRec<g1j> sh[TPB];
  static_assert(TPB == LB_KZG_MSM_NB / 2, "one lane per bucket with the bit set");
  const uint32_t job = blockIdx.y, k = blockIdx.x, m = threadIdx.x;  // k < 8 (grid)
  g1j acc;
  jac_set_inf(acc);
  if (k < 7 || m == 0) {
    const uint32_t low = m & ((1u << k) - 1u), high = m >> k;
    const uint32_t d = k < 7 ? (high << (k + 1)) | (1u << k) | low : LB_KZG_MSM_NB;  // 1 <= d <= 128
    acc = bsum[job * LB_KZG_MSM_NB + d - 1];
  }
  kzg_wave_sum(sh, acc);
  if (m == 0) G[job * 8 + k] = sh[0].v;
}

// One lane per job: sum_k 2^k G_k by Horner (7 doublings), compressed; 48 zero bytes for a
// job with a status
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_msm_final(uint32_t n_jobs, const g1j* __restrict__ G,
                                                                    const uint8_t* __restrict__ status,
                                                                    uint8_t* __restrict__ out48) {
  const uint32_t job = blockIdx.x * blockDim.x + threadIdx.x;
  if (job >= n_jobs) return;
  uint8_t* o = out48 + (size_t)job * 48;
  if (status[job] != LB_KZG_OK) {
    for (int i = 0; i < 48; i++) o[i] = 0;
    return;
  }
  g1j acc = G[job * 8 + 7];
#pragma unroll 1
  for (int k = 6; k >= 0; k--) {
    jac_dbl(acc, acc);
    const g1j g = G[job * 8 + k];
    jac_add(acc, acc, g);
  }
  g1a a;
  jac_to_aff(a, acc);
  g1_compress(o, a);
}

}  // namespace lb
