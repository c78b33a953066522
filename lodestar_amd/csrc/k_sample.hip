// Balance-weighted sampling over the swap-or-not shuffle (lb_sample_by_balance): the epoch's
// proposers and the next sync committee, chosen where the lists and the balance table lie.
//
// Reference: computeProposers / computeProposerIndex and getNextSyncCommitteeIndices
// (state-transition/src/util/seed.ts:22-80, 92-126), both the spec's rejection sampling
//   cand = active[compute_shuffled_index(i mod n, n, seed)]
//   rand = SHA256(seed || LE64(i div 32))[i mod 32]
//   accepted iff inc[cand] * 255 >= max_inc * rand
// over i = 0, 1, 2, ...  (include/lodestar_bls.h states the whole walk).
//
// The shuffle kernels of k_lists.hip hash a round's ceil(n/256) source digests for all n
// positions of one seed; the sampler wants a few to a few hundred positions of up to 64 seeds,
// so a candidate walks its 90 rounds with one SHA-256 block per round and no table.  A pass
// examines candidates [base, base + P) of every unfilled seed: k_sample_candidates writes each
// one's validator index and accept flag, k_sample_select compacts the accepted ones in order of
// i behind what the seed has already found.  The host reads the found counts between passes.
#include "bls_hash.h"
#include "bls_kernels.h"

namespace lb {

// words 0..7 of every block the sampler hashes: the seed, big-endian
LB_DEV void sample_seed_words(uint32_t w[8], const uint8_t* __restrict__ seed) {
  for (int i = 0; i < 8; i++)
    w[i] = ((uint32_t)seed[4 * i] << 24) | ((uint32_t)seed[4 * i + 1] << 16) | ((uint32_t)seed[4 * i + 2] << 8) |
           (uint32_t)seed[4 * i + 3];
}

// The largest of active[0..n) into *max_index (zeroed by the host): the host refuses the call
// when it is not below the balance table's size, whichever candidates get examined.
__global__ void __launch_bounds__(LB_LISTS_TPB) k_sample_range(uint32_t n, const uint32_t* __restrict__ active,
                                                               uint32_t* __restrict__ max_index) {
  uint32_t m = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t v = active[i];
    m = v > m ? v : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = __shfl_xor(m, o, 64);
    m = other > m ? other : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(max_index, m);
}

// Thread t < n_seeds x 90: pivots[s][r] = LE64(SHA256(seed_s || r)[0..8]) mod n
__global__ void __launch_bounds__(LB_LISTS_TPB) k_sample_pivots(uint32_t n_seeds, uint32_t n,
                                                                const uint8_t* __restrict__ seeds,
                                                                uint32_t* __restrict__ pivots) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_seeds * LB_SHUFFLE_ROUNDS) return;
  const uint32_t s = t / LB_SHUFFLE_ROUNDS, r = t - s * LB_SHUFFLE_ROUNDS;
  sha_block blk;
  blk.clear();
  sample_seed_words(blk.w, seeds + (size_t)s * 32);
  blk.w[8] = (r << 24) | 0x800000u;
  blk.w[15] = 33 * 8;
  uint32_t st[8];
  sha256_init(st);
  sha256_compress(st, blk.w);
  const uint64_t v = (uint64_t)__builtin_bswap32(st[0]) | ((uint64_t)__builtin_bswap32(st[1]) << 32);
  pivots[t] = (uint32_t)(v % n);
}

// Thread j < P of seed s = blockIdx.y: candidate i = base + j.  compute_shuffled_index(i mod n)
// with the arithmetic of k_shuffle_apply, the source digest of pos >> 8 hashed in place (seed ||
// r || LE32(pos >> 8): 37 bytes, one block); then the candidate's random byte and the test.  The
// random digest is the same for the 32 candidates of a group, which are 32 neighbouring lanes
// running it in lockstep: a wave spends one block on it either way.  A seed that has filled,
// and a candidate at or past max_candidates, are left alone (flag 0).  An index outside the
// balance table reads as increment 0; the host refuses such a call from k_sample_range's word.
__global__ void __launch_bounds__(LB_LISTS_TPB)
    k_sample_candidates(uint32_t n, uint32_t count, uint32_t base, uint32_t pass, uint32_t max_candidates,
                        uint32_t max_inc, const uint8_t* __restrict__ seeds, const uint32_t* __restrict__ pivots,
                        const uint32_t* __restrict__ active, const uint8_t* __restrict__ inc, uint32_t inc_n,
                        const uint32_t* __restrict__ found, uint32_t* __restrict__ cand,
                        uint8_t* __restrict__ accept) {
  const uint32_t s = blockIdx.y;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= pass) return;
  const size_t at = (size_t)s * pass + j;
  const uint32_t i = base + j;
  if (found[s] >= count || i >= max_candidates) {
    accept[at] = 0;
    return;
  }
  sha_block blk;
  blk.clear();
  sample_seed_words(blk.w, seeds + (size_t)s * 32);
  blk.w[15] = 37 * 8;
  const uint32_t* __restrict__ pv = pivots + s * LB_SHUFFLE_ROUNDS;
  uint32_t st[8];
  uint32_t idx = i % n;
  for (uint32_t r = 0; r < LB_SHUFFLE_ROUNDS; r++) {
    uint32_t flip = pv[r] + n - idx;  // (pivot < n, idx < n <= 2^22: in (0, 2n), no wrap)
    if (flip >= n) flip -= n;
    const uint32_t pos = idx > flip ? idx : flip;
    const uint32_t k = pos >> 8;  // (< 2^14: LE32(k) is two bytes and two zeros)
    blk.w[8] = (r << 24) | ((k & 0xff) << 16) | (k & 0xff00);
    blk.w[9] = 0x800000u;
    sha256_init(st);
    sha256_compress(st, blk.w);
    const uint32_t b = (pos & 255) >> 3;  // the digest's byte
    const uint32_t byte = (st[b >> 2] >> (24 - 8 * (b & 3))) & 0xff;
    if ((byte >> (pos & 7)) & 1) idx = flip;
  }
  const uint32_t c = active[idx];
  // rand = SHA256(seed || LE64(i / 32))[i % 32]   (40 bytes; i / 32 < 2^17)
  blk.w[8] = __builtin_bswap32(i >> 5);
  blk.w[9] = 0;
  blk.w[10] = 0x80000000u;
  blk.w[15] = 40 * 8;
  sha256_init(st);
  sha256_compress(st, blk.w);
  const uint32_t b = i & 31;
  const uint32_t rnd = (st[b >> 2] >> (24 - 8 * (b & 3))) & 0xff;
  const uint32_t w = c < inc_n ? inc[c] : 0;
  cand[at] = c;
  accept[at] = w * 255u >= max_inc * rnd ? 1 : 0;
}

// One workgroup per seed: the pass's accepted candidates, in order of i, appended behind the
// seed's found[s] until it holds `count`.  A stretch of LB_LISTS_TPB candidates at a time: a
// ballot and popcount per wave, the waves' counts summed through LDS.  tried[s] = i + 1 of the
// candidate that filled the last place.
__global__ void __launch_bounds__(LB_LISTS_TPB)
    k_sample_select(uint32_t count, uint32_t base, uint32_t pass, const uint32_t* __restrict__ cand,
                    const uint8_t* __restrict__ accept, uint32_t* __restrict__ out, uint32_t* __restrict__ found,
                    uint32_t* __restrict__ tried) {
  constexpr uint32_t kWaves = LB_LISTS_TPB / 64;
  __shared__ uint32_t wave_cnt[kWaves];
  const uint32_t s = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t have = found[s];  // (uniform over the workgroup, as is every branch on it)
  if (have >= count) return;
  const uint32_t* __restrict__ c_s = cand + (size_t)s * pass;
  const uint8_t* __restrict__ a_s = accept + (size_t)s * pass;
  uint32_t* __restrict__ out_s = out + (size_t)s * count;
  for (uint32_t c0 = 0; c0 < pass && have < count; c0 += LB_LISTS_TPB) {
    const uint32_t j = c0 + threadIdx.x;
    const bool acc = j < pass && a_s[j] != 0;
    const unsigned long long mask = __ballot(acc);
    if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kWaves; w++) {
      const uint32_t v = wave_cnt[w];
      if (w < wave) before += v;
      total += v;
    }
    if (acc) {
      const uint32_t rank = have + before + (uint32_t)__popcll(mask & (((unsigned long long)1 << lane) - 1));
      if (rank < count) {
        out_s[rank] = c_s[j];
        if (rank == count - 1) tried[s] = base + j + 1;
      }
    }
    have += total;
    __syncthreads();  // (wave_cnt is rewritten by the next stretch)
  }
  if (threadIdx.x == 0) found[s] = have < count ? have : count;
}

}  // namespace lb
