// Device-resident index lists (lb_index_list_*, lb_verify_requests_keys*): an epoch's shuffling
// computed where the verifier reads it, and set descriptors ("this slice of that list, these
// bits") expanded into the validator indices the unchanged pipeline takes as pubkey_indices.
//
// Reference: unshuffleList(activeIndices, seed) under computeEpochShuffling
// (state-transition/src/util/shuffle.ts, epochShuffling.ts:62-101), which is
//   out[i] = active[compute_shuffled_index(i, n, seed)]
// of the consensus spec's swap-or-not shuffle; and
// aggregationBits.intersectValues(getBeaconCommittee(slot, index)) (cache/epochCache.ts:684-685).
//
// The shuffle in two kernels.  Every round's pivot and its ceil(n/256) source digests depend on
// (seed, round, position >> 8) alone, so k_shuffle_sources hashes them once -- 90 x ceil(n/256)
// SHA-256 blocks and 90 64-bit remainders in all -- and k_shuffle_apply walks one position
// through the 90 rounds with an add, a conditional subtract, a max, one byte load and a bit test
// per round: no hash and no division per element.
#include "bls_hash.h"
#include "bls_kernels.h"

namespace lb {

// Thread t < 90 x nblk: digest k = t % nblk of round r = t / nblk,
//   table[r][32 k ..] = SHA256(seed || r || LE32(k))   (37 bytes: one block)
// and, from the thread of k == 0, pivots[r] = LE64(SHA256(seed || r)[0..8]) mod n.
__global__ void __launch_bounds__(LB_LISTS_TPB) k_shuffle_sources(uint32_t n, const uint8_t* __restrict__ seed,
                                                                  uint32_t* __restrict__ pivots,
                                                                  uint32_t* __restrict__ table) {
  const uint32_t nblk = (n + 255) / 256;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= LB_SHUFFLE_ROUNDS * nblk) return;
  const uint32_t r = t / nblk, k = t - r * nblk;
  sha_block blk;
  blk.clear();
  for (int i = 0; i < 32; i++) blk.put(i, seed[i]);
  blk.put(32, (uint8_t)r);
  uint32_t st[8];
  if (k == 0) {
    sha_block pv = blk;
    pv.put(33, 0x80);
    pv.w[15] = 33 * 8;
    sha256_init(st);
    sha256_compress(st, pv.w);
    const uint64_t v = (uint64_t)__builtin_bswap32(st[0]) | ((uint64_t)__builtin_bswap32(st[1]) << 32);
    pivots[r] = (uint32_t)(v % n);
  }
  for (int i = 0; i < 4; i++) blk.put(33 + i, (uint8_t)(k >> (8 * i)));
  blk.put(37, 0x80);
  blk.w[15] = 37 * 8;
  sha256_init(st);
  sha256_compress(st, blk.w);
  // (the digest's bytes in order: its big-endian words byte-swapped into little-endian stores)
  uint32_t* out = table + ((size_t)r * nblk + k) * 8;
  for (int i = 0; i < 8; i++) out[i] = __builtin_bswap32(st[i]);
}

// Thread i < n: compute_shuffled_index(i, n, seed) over the precomputed sources, then the
// gather out[i] = active[that].  Bit `pos` of round r's row is byte pos >> 3 of the row (digest
// pos >> 8, its byte (pos & 255) >> 3), bit pos & 7.
__global__ void __launch_bounds__(LB_LISTS_TPB) k_shuffle_apply(uint32_t n, const uint32_t* __restrict__ pivots,
                                                                const uint8_t* __restrict__ table,
                                                                const uint32_t* __restrict__ active,
                                                                uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t row = shuffle_row_bytes(n);
  uint32_t idx = i;
  for (uint32_t r = 0; r < LB_SHUFFLE_ROUNDS; r++) {
    uint32_t flip = pivots[r] + n - idx;  // (pivot < n, idx < n <= 2^22: in (0, 2n), no wrap)
    if (flip >= n) flip -= n;
    const uint32_t pos = idx > flip ? idx : flip;
    const uint32_t byte = table[r * row + (pos >> 3)];
    if ((byte >> (pos & 7)) & 1) idx = flip;
  }
  out[i] = active[idx];
}

// One wave per set: idx[pk_off[s] ..) = the set's validator indices in list order.  The host
// has checked every bound the reads depend on (list id and size, a + len, the pool, the bits'
// bytes) and pk_off holds its counts of the same bits; a write is still fenced to the set's own
// range [pk_off[s], pk_off[s+1]).
//   DIRECT  one index, the descriptor's own
//   SLICE   a copy of pool[a .. a + len)
//   BITS    lane l takes bits [64 l, 64 l + 64) of a 4,096-bit stretch, assembled from bytes
//           (bits_off is a byte offset of no alignment) and masked to len; a wave prefix sum
//           of the popcounts ranks each lane's members; longer sets loop with a carried base
__global__ void __launch_bounds__(LB_LISTS_TPB) k_expand_keys(uint32_t n_sets, const lb_set_keys* __restrict__ sets,
                                                              const uint32_t* __restrict__ pool,
                                                              const uint8_t* __restrict__ bits, IndexLists lists,
                                                              const uint32_t* __restrict__ pk_off,
                                                              uint32_t* __restrict__ idx) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * (LB_LISTS_TPB / 64) + (threadIdx.x >> 6);
  if (s >= n_sets) return;
  const lb_set_keys d = sets[s];
  const uint32_t begin = pk_off[s], end = pk_off[s + 1];
  if (d.kind == LB_KEYS_DIRECT) {
    if (lane == 0 && begin < end) idx[begin] = d.a;
    return;
  }
  if (d.kind == LB_KEYS_SLICE) {
    for (uint32_t t = lane; t < d.len && begin + t < end; t += 64) idx[begin + t] = pool[d.a + t];
    return;
  }
  if (d.kind != LB_KEYS_BITS || d.list >= LB_INDEX_LISTS) return;
  const uint32_t* __restrict__ list = lists.d[d.list] + d.a;
  const uint8_t* __restrict__ sb = bits + d.bits_off;
  uint32_t base = begin;
  for (uint32_t c = 0; c < d.len; c += 64 * 64) {
    const uint32_t first = c + 64 * lane;  // this lane's first bit
    const uint32_t nb = first >= d.len ? 0 : (d.len - first < 64 ? d.len - first : 64);
    uint64_t w = 0;
    for (uint32_t b = 0; b < (nb + 7) / 8; b++) w |= (uint64_t)sb[first / 8 + b] << (8 * b);
    if (nb < 64) w &= ((uint64_t)1 << nb) - 1;  // (nb == 0: w is 0 already)
    const uint32_t cnt = (uint32_t)__popcll(w);
    uint32_t incl = cnt;  // inclusive prefix sum over the wave
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if ((int)lane >= o) incl += up;
    }
    uint32_t at = base + incl - cnt;
    while (w) {
      const uint32_t j = (uint32_t)__builtin_ctzll(w);
      w &= w - 1;
      if (at < end) idx[at] = list[first + j];
      at++;
    }
    base += __shfl(incl, 63, 64);
  }
}

}  // namespace lb
