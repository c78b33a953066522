// Blob KZG proof verification (deneb verify_blob_kzg_proof_batch): everything over the
// scalar field Fr, and the pairing tail on the existing G1 / pairing routines.
//
// Reference: ckzg.verifyBlobKzgProofBatch on block import
// (packages/beacon-node/src/chain/validation/blobSidecar.ts:195-217); semantics after
// consensus-specs deneb polynomial-commitments.md.  The two domain separators below are
// the spec's FIAT_SHAMIR_PROTOCOL_DOMAIN and RANDOM_CHALLENGE_KZG_BATCH_DOMAIN; they
// live here and nowhere else on the device side.
//
//   k_kzg_roots    once per context : roots[i] = omega^brp(i), Montgomery form, in HBM
//   k_kzg_hash     workgroup / blob : z = hash_to_bls_field(transcript), 2,050 chained
//                                     compressions; schedules expanded a tile ahead
//   k_kzg_eval     workgroup / blob : y = f(z), barycentric, one inversion per thread
//   k_kzg_decode   lane / point     : validate_kzg_g1 of commitments and proofs
//   k_kzg_rho      one wave         : statuses, rho and the ladders' scalars
//   k_kzg_ladder   lane / ladder    : 255-bit G1 ladders (jac_mul_be32)
//   k_jac_sum / k_kzg_each_sum      : A and B of the pairing check
//   k_kzg_miller   lane / pair      : Miller(A, -[tau]_2), Miller(B, G2)
//   k_kzg_final    lane / check     : product, final exponentiation, == 1
#include "bls_kzg.h"

namespace lb {

__device__ __constant__ const char KZG_FS_DOMAIN[17] = "FSBLOBVERIFY_V1_";
__device__ __constant__ const char KZG_RC_DOMAIN[17] = "RCKZGBATCH___V1_";

LB_DEV uint32_t kzg_domain_word(const char* d, uint32_t j) {
  return ((uint32_t)(uint8_t)d[4 * j] << 24) | ((uint32_t)(uint8_t)d[4 * j + 1] << 16) |
         ((uint32_t)(uint8_t)d[4 * j + 2] << 8) | (uint32_t)(uint8_t)d[4 * j + 3];
}

// ---- setup ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kzg_roots(fr* __restrict__ roots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= LB_KZG_N) return;
  const uint32_t e = __brev(i) >> 20;  // 12-bit reversal
  fr w, acc;
  fr_set(w, LB_FR_OMEGA);
  fr_one(acc);
#pragma unroll 1
  for (int b = 11; b >= 0; b--) {
    fr_sqr(acc, acc);
    if ((e >> b) & 1u) fr_mul(acc, acc, w);
  }
  roots[i] = acc;
}

// [tau]_2 -> -[tau]_2 (affine); status = LB_ST_*, LB_ST_PK_INFINITY for the point at infinity
__global__ void __launch_bounds__(TPB) k_kzg_setup_g2(const uint8_t* __restrict__ in96, g2a* __restrict__ neg_tau,
                                                      uint8_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  g2a q;
  uint8_t st = g2_deserialize(q, in96, 96);
  if (st == LB_ST_OK && q.inf) st = LB_ST_PK_INFINITY;
  if (st == LB_ST_OK) {
    g2j j;
    jac_from_aff(j, q);
    if (!g2_in_subgroup(j)) st = LB_ST_NOT_IN_GROUP;
  }
  if (st == LB_ST_OK) {
    fp2_neg(q.y, q.y);
    neg_tau[0] = q;
  }
  status[0] = st;
}

// ---- Fiat-Shamir challenge ----------------------------------------------------
// Word j (big-endian) of compute_challenge's padded transcript:
//   "FSBLOBVERIFY_V1_" | BE128(4096) | blob | commitment | 0x80 0... | BE64(bit length)
LB_DEV uint32_t kzg_fs_word(const uint32_t* __restrict__ blob_w, const uint32_t* __restrict__ com_w, uint32_t j) {
  if (j < 4) return kzg_domain_word(KZG_FS_DOMAIN, j);
  if (j < 8) return j == 7 ? LB_KZG_N : 0u;
  if (j < 8 + 8 * LB_KZG_N) return __builtin_bswap32(blob_w[j - 8]);
  j -= 8 + 8 * LB_KZG_N;
  if (j < 12) return __builtin_bswap32(com_w[j]);
  if (j == 12) return 0x80000000u;
  if (j == 23) return (32u + LB_KZG_BLOB_BYTES + 48u) * 8u;  // (16 LB_KZG_FS_BLOCKS - 1 - 8 - 8 LB_KZG_N)
  return 0u;
}

static constexpr uint32_t KZG_TILE = 64;  // SHA blocks per tile: one per lane of the expanding wave

// One workgroup per blob.  The chain of 2,050 compressions is serial, but a block's message
// schedule depends on the message alone: wave 1 loads a tile of 64 blocks (one per lane),
// byte-swaps it and expands W[0..63] + K into LDS (word-major, so the lanes' stores hit
// distinct banks) while lane 0 of wave 0 runs the 64 rounds of the previous tile's blocks
// out of the other buffer.  A block holds two whole field elements (the 32-byte header
// keeps them aligned), so the lane that loads it also tests them against r.
__global__ void __launch_bounds__(LB_KZG_HASH_TPB) k_kzg_hash(const uint8_t* __restrict__ blobs,
                                                              const uint8_t* __restrict__ com48,
                                                              uint8_t* __restrict__ z32, uint8_t* __restrict__ status) {
  __shared__ uint32_t sh[2][64][KZG_TILE];
  __shared__ uint32_t s_bad;
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* blob_w = reinterpret_cast<const uint32_t*>(blobs + (size_t)b * LB_KZG_BLOB_BYTES);
  const uint32_t* com_w = reinterpret_cast<const uint32_t*>(com48 + (size_t)b * 48);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  const uint32_t n_tiles = (LB_KZG_FS_BLOCKS + KZG_TILE - 1) / KZG_TILE;
  uint32_t st[8];
  sha256_init(st);
  for (uint32_t t = 0; t <= n_tiles; t++) {
    if (tid >= 64 && t < n_tiles) {  // expand tile t
      const uint32_t lane = tid - 64, blk = t * KZG_TILE + lane;
      if (blk < LB_KZG_FS_BLOCKS) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; i++) w[i] = kzg_fs_word(blob_w, com_w, 16 * blk + i);
        // elements 2 blk - 1 (words 0..7) and 2 blk (words 8..15)
        uint32_t tl[8];
        bool bad = false;
        if (blk >= 1 && blk <= LB_KZG_N / 2) {
#pragma unroll
          for (int j = 0; j < 8; j++) tl[j] = w[7 - j];
          bad |= !fr_raw_is_canonical(tl);
        }
        if (blk < LB_KZG_N / 2) {
#pragma unroll
          for (int j = 0; j < 8; j++) tl[j] = w[15 - j];
          bad |= !fr_raw_is_canonical(tl);
        }
        if (bad) atomicOr(&s_bad, 1u);
        uint32_t(*dst)[KZG_TILE] = sh[t & 1];
#pragma unroll
        for (int i = 0; i < 64; i++) {
          uint32_t wi;
          if (i < 16) {
            wi = w[i];
          } else {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const uint32_t s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
            wi = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
            w[i & 15] = wi;
          }
          dst[i][lane] = wi + SHA_K[i];
        }
      }
    } else if (tid == 0 && t > 0) {  // the rounds of tile t - 1
      const uint32_t(*src)[KZG_TILE] = sh[(t - 1) & 1];
      const uint32_t first = (t - 1) * KZG_TILE;
      const uint32_t cnt = LB_KZG_FS_BLOCKS - first < KZG_TILE ? LB_KZG_FS_BLOCKS - first : KZG_TILE;
#pragma unroll 1
      for (uint32_t k = 0; k < cnt; k++) {
        uint32_t a = st[0], bb = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 8
        for (int i = 0; i < 64; i++) {
          const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
          const uint32_t ch = (e & f) ^ (~e & g);
          const uint32_t t1 = h + S1 + ch + src[i][k];
          const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
          const uint32_t mj = (a & bb) ^ (a & c) ^ (bb & c);
          h = g;
          g = f;
          f = e;
          e = d + t1;
          d = c;
          c = bb;
          bb = a;
          a = t1 + S0 + mj;
        }
        st[0] += a;
        st[1] += bb;
        st[2] += c;
        st[3] += d;
        st[4] += e;
        st[5] += f;
        st[6] += g;
        st[7] += h;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool bad = s_bad != 0;
    uint8_t* o = z32 + (size_t)b * 32;
    if (bad) {
      for (int i = 0; i < 32; i++) o[i] = 0;
    } else {
      fr z;
      fr_from_be_words_reduce(z, st);
      fr_to_be32(o, z);
    }
    status[b] = bad ? LB_KZG_BAD_BLOB : LB_KZG_OK;
  }
}

// ---- evaluation ---------------------------------------------------------------
// y = f(z) for the blob's polynomial in evaluation form over roots[] (brp order):
//   z == roots[i]: f[i];  else (z^N - 1) / N * sum_i f[i] roots[i] / (z - roots[i]).
// One workgroup per blob; thread t owns elements t, t + 256, ... (16 of them: a wave's
// loads of roots[] and of the blob are contiguous), inverts its 16 differences with
// Montgomery's trick (one Fr inversion per thread) and accumulates its terms; an LDS tree
// sums the 256 partials.  status: kept when already set, else LB_KZG_BAD_BLOB (an element
// >= r) or LB_KZG_BAD_SCALAR (z >= r); y of such an item is zero bytes.
__global__ void __launch_bounds__(LB_KZG_EVAL_TPB) k_kzg_eval(const uint8_t* __restrict__ blobs,
                                                              const fr* __restrict__ roots,
                                                              const uint8_t* __restrict__ z32,
                                                              uint8_t* __restrict__ y32, uint8_t* __restrict__ status) {
  constexpr int STRIP = LB_KZG_N / LB_KZG_EVAL_TPB;
  __shared__ fr sh[LB_KZG_EVAL_TPB];
  __shared__ uint32_t s_eq, s_bad;
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint32_t* blob_w = reinterpret_cast<const uint32_t*>(blobs + (size_t)b * LB_KZG_BLOB_BYTES);
  if (tid == 0) {
    s_eq = 0xffffffffu;
    s_bad = 0;
  }
  __syncthreads();
  fr z;
  const bool z_ok = kzg_load_fr(z, reinterpret_cast<const uint32_t*>(z32 + (size_t)b * 32));
  fr one;
  fr_one(one);
  // forward: prefix products of the differences (a zero difference -- z is that root -- is
  // replaced by 1: the sum is not used then)
  fr pre[STRIP];
  fr run = one;
#pragma unroll
  for (int k = 0; k < STRIP; k++) {
    const uint32_t i = tid + (uint32_t)k * LB_KZG_EVAL_TPB;
    const fr w = roots[i];
    fr d;
    fr_sub(d, z, w);
    if (fr_is_zero(d)) {
      s_eq = i;  // (the roots are distinct: at most one writer)
      d = one;
    }
    fr_mul(run, run, d);
    pre[k] = run;
  }
  fr inv;
  fr_inv(inv, run);
  // backward: 1 / d_k = inv * pre[k - 1], inv *= d_k
  fr sum;
  fr_zero(sum);
  bool bad = false;
#pragma unroll
  for (int k = STRIP - 1; k >= 0; k--) {
    const uint32_t i = tid + (uint32_t)k * LB_KZG_EVAL_TPB;
    const fr w = roots[i];
    fr d, ik, f, t;
    fr_sub(d, z, w);
    if (fr_is_zero(d)) d = one;
    if (k > 0)
      fr_mul(ik, inv, pre[k > 0 ? k - 1 : 0]);
    else
      ik = inv;
    fr_mul(inv, inv, d);
    bad |= !kzg_load_fr(f, blob_w + 8 * i);
    fr_mul(t, f, w);
    fr_mul(t, t, ik);
    fr_add(sum, sum, t);
  }
  if (bad) atomicOr(&s_bad, 1u);
  sh[tid] = sum;
  __syncthreads();
  for (uint32_t s = LB_KZG_EVAL_TPB / 2; s > 0; s >>= 1) {
    if (tid < s) {
      fr m = sh[tid], o = sh[tid + s];
      fr_add(m, m, o);
      sh[tid] = m;
    }
    __syncthreads();
  }
  if (tid == 0) {
    uint8_t st = status[b];
    if (st == LB_KZG_OK && s_bad) st = LB_KZG_BAD_BLOB;
    if (st == LB_KZG_OK && !z_ok) st = LB_KZG_BAD_SCALAR;
    uint8_t* o = y32 + (size_t)b * 32;
    if (st != LB_KZG_OK) {
      for (int i = 0; i < 32; i++) o[i] = 0;
    } else if (s_eq != 0xffffffffu) {
      fr f;
      kzg_load_fr(f, blob_w + 8 * s_eq);
      fr_to_be32(o, f);
    } else {
      fr zn = z, y;
#pragma unroll 1
      for (int k = 0; k < 12; k++) fr_sqr(zn, zn);  // z^4096
      fr_sub(zn, zn, one);
      fr_mul_const(zn, zn, LB_FR_NINV);
      fr_mul(y, zn, sh[0]);
      fr_to_be32(o, y);
    }
    status[b] = st;
  }
}

// ---- tail -----------------------------------------------------------------------
// validate_kzg_g1: P[i] = C_i, P[n + i] = pi_i (infinity when refused), P[2n] = G1
__global__ void __launch_bounds__(TPB) k_kzg_decode(uint32_t n, const uint8_t* __restrict__ com48,
                                                    const uint8_t* __restrict__ proofs48, g1j* __restrict__ P,
                                                    uint8_t* __restrict__ pt_status) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > 2 * n) return;
  g1j j;
  if (i == 2 * n) {
    fp_set(j.X, LB_G1_X);
    fp_set(j.Y, LB_G1_Y);
    fp_one(j.Z);
    P[i] = j;
    return;
  }
  const uint8_t* src = i < n ? com48 + (size_t)i * 48 : proofs48 + (size_t)(i - n) * 48;
  g1a a;
  uint8_t st = g1_deserialize(a, src, 48);
  if (st == LB_ST_OK) {
    jac_from_aff(j, a);
    if (!g1_in_subgroup(j)) st = LB_ST_NOT_IN_GROUP;
  }
  if (st != LB_ST_OK) jac_set_inf(j);
  P[i] = j;
  pt_status[i] = st;
}

static constexpr uint32_t KZG_RC_WORDS = 8 + 40 * LB_KZG_MAX_BLOBS;  // header + items

// One wave.  Lane i < n settles item i's status (kept when already set; then z or y >= r,
// then the commitment, then the proof) and lays its 160 transcript bytes into LDS; lane 0
// hashes  "RCKZGBATCH___V1_" | BE64(4096) | BE64(n) | (C_i | z_i | y_i | pi_i)...  into rho;
// lane i then writes the scalars of its ladders, 32 bytes big-endian each:
//   batch:  [i] rho^i   [n + i] rho^i z_i   [2n + i] rho^i   [3n] -(sum rho^i y_i)
//   each :  [i] z_i     [n + i] -y_i
// skip[0] = 1 when any status is set (batch mode: no ladder, no pairing).
__global__ void __launch_bounds__(TPB) k_kzg_rho(uint32_t n, uint32_t mode, const uint8_t* __restrict__ com48,
                                                 const uint8_t* __restrict__ proofs48,
                                                 const uint8_t* __restrict__ z32, const uint8_t* __restrict__ y32,
                                                 const uint8_t* __restrict__ pt_status, uint8_t* __restrict__ status,
                                                 uint8_t* __restrict__ scalars, uint8_t* __restrict__ skip) {
  __shared__ uint32_t msg[KZG_RC_WORDS + 32];
  __shared__ fr s_rho;
  __shared__ fr s_part[TPB];
  const uint32_t i = threadIdx.x;
  if (blockIdx.x != 0 || n > LB_KZG_MAX_BLOBS) return;
  fr z, y;
  fr_zero(z);
  fr_zero(y);
  bool bad = false;
  if (i < n) {
    const uint32_t* zw = reinterpret_cast<const uint32_t*>(z32 + (size_t)i * 32);
    const uint32_t* yw = reinterpret_cast<const uint32_t*>(y32 + (size_t)i * 32);
    const bool ok = kzg_load_fr(z, zw) & kzg_load_fr(y, yw);
    uint8_t st = status[i];
    if (st == LB_KZG_OK && !ok) st = LB_KZG_BAD_SCALAR;
    if (st == LB_KZG_OK && pt_status[i] != LB_ST_OK) st = LB_KZG_BAD_COMMITMENT;
    if (st == LB_KZG_OK && pt_status[n + i] != LB_ST_OK) st = LB_KZG_BAD_PROOF;
    status[i] = st;
    bad = st != LB_KZG_OK;
    if (mode == LB_KZG_BATCH) {
      uint32_t* m = msg + 8 + 40 * i;
      const uint32_t* cw = reinterpret_cast<const uint32_t*>(com48 + (size_t)i * 48);
      const uint32_t* pw = reinterpret_cast<const uint32_t*>(proofs48 + (size_t)i * 48);
      for (int k = 0; k < 12; k++) m[k] = __builtin_bswap32(cw[k]);
      for (int k = 0; k < 8; k++) m[12 + k] = __builtin_bswap32(zw[k]);
      for (int k = 0; k < 8; k++) m[20 + k] = __builtin_bswap32(yw[k]);
      for (int k = 0; k < 12; k++) m[28 + k] = __builtin_bswap32(pw[k]);
    }
  }
  const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;
  if (i == 0) skip[0] = any_bad ? 1 : 0;
  if (mode == LB_KZG_EACH) {
    if (i < n) {
      fr ny;
      fr_neg(ny, y);
      fr_to_be32(scalars + (size_t)i * 32, z);
      fr_to_be32(scalars + (size_t)(n + i) * 32, ny);
    }
    return;
  }
  if (any_bad) return;
  if (i == 0) {
    for (uint32_t k = 0; k < 4; k++) msg[k] = kzg_domain_word(KZG_RC_DOMAIN, k);
    msg[4] = 0;
    msg[5] = LB_KZG_N;
    msg[6] = 0;
    msg[7] = n;
    const uint32_t words = 8 + 40 * n;  // message words; then 0x80, zeros, the bit length
    const uint32_t blocks = (words + 3 + 15) / 16;
    for (uint32_t k = words; k < 16 * blocks; k++) msg[k] = 0;
    msg[words] = 0x80000000u;
    msg[16 * blocks - 1] = words * 32u;
    uint32_t st[8];
    sha256_init(st);
#pragma unroll 1
    for (uint32_t k = 0; k < blocks; k++) sha256_compress(st, msg + 16 * k);
    fr rho;
    fr_from_be_words_reduce(rho, st);
    s_rho = rho;
  }
  __syncthreads();
  fr t;
  fr_zero(t);
  if (i < n) {
    const fr rho = s_rho;
    fr ri;
    fr_one(ri);
#pragma unroll 1
    for (int bit = 6; bit >= 0; bit--) {  // rho^i, i <= 63
      fr_sqr(ri, ri);
      if ((i >> bit) & 1u) fr_mul(ri, ri, rho);
    }
    fr rz;
    fr_mul(rz, ri, z);
    fr_mul(t, ri, y);
    fr_to_be32(scalars + (size_t)i * 32, ri);
    fr_to_be32(scalars + (size_t)(n + i) * 32, rz);
    fr_to_be32(scalars + (size_t)(2 * n + i) * 32, ri);
  }
  s_part[i] = t;
  __syncthreads();
  if (i == 0) {
    fr s;
    fr_zero(s);
#pragma unroll 1
    for (uint32_t k = 0; k < n; k++) {
      const fr p = s_part[k];
      fr_add(s, s, p);
    }
    fr_neg(s, s);
    fr_to_be32(scalars + (size_t)(3 * n) * 32, s);
  }
}

// One 255-bit ladder per lane (the layout k_kzg_rho describes); out[j] = [scalar_j] point_j
__global__ void __launch_bounds__(TPB, LB_W_SCALAR) k_kzg_ladder(uint32_t n, uint32_t mode,
                                                                 const g1j* __restrict__ P,
                                                                 const uint8_t* __restrict__ scalars,
                                                                 const uint8_t* __restrict__ skip,
                                                                 g1j* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t jobs = mode == LB_KZG_BATCH ? 3 * n + 1 : 2 * n;
  if (j >= jobs || (mode == LB_KZG_BATCH && skip[0])) return;
  uint32_t pt;
  if (mode == LB_KZG_BATCH)
    pt = j < n ? n + j : j < 2 * n ? j : j < 3 * n ? j - 2 * n : 2 * n;
  else
    pt = j < n ? n + j : 2 * n;
  uint8_t k[32];
  for (int b = 0; b < 32; b++) k[b] = scalars[(size_t)j * 32 + b];
  const g1j p = P[pt];
  g1j r;
  jac_mul_be32(r, p, k);
  out[j] = r;
}

// per-item pairs: AB[2i] = pi_i, AB[2i + 1] = C_i - [y_i]G1 + [z_i]pi_i
__global__ void __launch_bounds__(TPB) k_kzg_each_sum(uint32_t n, const g1j* __restrict__ P,
                                                      const g1j* __restrict__ lad, g1j* __restrict__ AB) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1j s = P[i], t = lad[i];
  jac_add(s, s, t);
  t = lad[n + i];
  jac_add(s, s, t);
  AB[2 * i] = P[n + i];
  AB[2 * i + 1] = s;
}

// f[t] = Miller(AB[t], Q), Q = -[tau]_2 for even t (the A side), the G2 generator for odd t
// (the B side); a pair whose G1 side is infinity contributes 1
__global__ void __launch_bounds__(TPB, LB_W_TAIL) k_kzg_miller(uint32_t m, const g1j* __restrict__ AB,
                                                               const g2a* __restrict__ neg_tau,
                                                               const uint8_t* __restrict__ skip,
                                                               fp12* __restrict__ f) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * m || (skip && skip[0])) return;
  const g1j pj = AB[t];
  g1a p;
  jac_to_aff(p, pj);
  g2a q;
  if (t & 1u) {
    fp2_set(q.x, LB_G2_X);
    fp2_set(q.y, LB_G2_Y);
    q.inf = false;
  } else {
    q = neg_tau[0];
  }
  fp12 r;
  fp12_one(r);
  if (!p.inf) miller_loop(r, p, q);
  f[t] = r;
}

// verdict[c] = (f[2c] f[2c + 1])^((p^12 - 1) / r) == 1; an item with a status (each mode),
// or a skipped batch, is 0
__global__ void __launch_bounds__(TPB, LB_W_TAIL) k_kzg_final(uint32_t m, uint32_t mode, const fp12* __restrict__ f,
                                                              const uint8_t* __restrict__ status,
                                                              const uint8_t* __restrict__ skip,
                                                              uint8_t* __restrict__ verdict) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  if (mode == LB_KZG_BATCH ? skip[0] != 0 : status[c] != LB_KZG_OK) {
    verdict[c] = 0;
    return;
  }
  fp12 a = f[2 * c], r;
  {
    const fp12 b = f[2 * c + 1];
    fp12_mul(a, a, b);
  }
  final_exp(r, a);
  verdict[c] = fp12_is_one(r) ? 1 : 0;
}

}  // namespace lb
