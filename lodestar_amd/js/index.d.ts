// Type declarations for lodestar_amd/js/bls_gpu_verifier.js: the GPU verifier as a
// Lodestar IBlsVerifier (packages/beacon-node/src/chain/bls/interface.ts:4-68), so a
// TypeScript beacon node can construct it where chain.ts:206-208 picks the bls pool.
// Signature sets follow @lodestar/state-transition's ISignatureSet
// (packages/state-transition/src/util/signatureSets.ts:5-24); a pubkey may be given by
// validator index ({index}) once syncPubkeys() has mirrored index2pubkey on the GPUs.

/** @chainsafe/bls PointFormat (the reference serializes with PointFormat.uncompressed,
 * BN/chain/bls/multithread/index.ts:144 -> jobItem.ts:59). */
export type PointFormat = "compressed" | "uncompressed";
export const PointFormat: {compressed: "compressed"; uncompressed: "uncompressed"};
/** The shape of a @chainsafe/bls PublicKey this verifier needs: toBytes(format) returns the
 * compressed 48-byte encoding unless format is "uncompressed" (96 bytes). */
export type PublicKeyLike = {toBytes(format?: PointFormat): Uint8Array};
/** A public key: a @chainsafe/bls PublicKey (as index2pubkey holds them; shipped as its
 * validator index once syncPubkeys/syncIndex2pubkey mirrored it, else serialized with
 * toBytes("uncompressed")), its 96-byte uncompressed or 48-byte compressed encoding, or
 * {index}: a validator index into the GPUs' pubkey tables. */
export type GpuPublicKey = PublicKeyLike | Uint8Array | {index: number};

/** signatureSets.ts:5-24 */
export type SingleSignatureSet = {
  type: "single";
  pubkey: GpuPublicKey;
  signingRoot: Uint8Array;
  signature: Uint8Array;
};
export type AggregatedSignatureSet = {
  type: "aggregate";
  pubkeys: GpuPublicKey[];
  signingRoot: Uint8Array;
  signature: Uint8Array;
};
/** An aggregate set over a committee held on the GPU: its keys are list[start + j] for every set
 * bit j < length of `bits` (SSZ bit order, any delimiter bit stripped), `list` an index list
 * loaded with syncShuffling / putIndexList -- the attestation as it arrived, in place of
 * aggregationBits.intersectValues(getBeaconCommittee(slot, index)) (epochCache.ts:684-685). */
export type BitsSignatureSet = {
  type: "bits";
  list: number;
  start: number;
  length: number;
  bits: Uint8Array;
  signingRoot: Uint8Array;
  signature: Uint8Array;
};
export type ISignatureSet = SingleSignatureSet | AggregatedSignatureSet | BitsSignatureSet;

/** interface.ts:4-23 */
export type VerifySignatureOpts = {
  batchable?: boolean;
  /** here: the device's priority lane at once (no queue, no JS main-thread blocking) */
  verifyOnMainThread?: boolean;
  /** here: queue front, then the device's priority lane (lb_verify_requests_priority_async) */
  priority?: boolean;
};

/** interface.ts:25-75 */
export interface IBlsVerifier {
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  verifySignatureSetsSameMessage(
    sets: {publicKey: GpuPublicKey; signature: Uint8Array}[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<boolean[]>;
  close(): Promise<void>;
  canAcceptWork(): boolean;
}

/** The addon's batch (include/lodestar_bls.h lb_request_batch). */
export type PackedRequests = {
  requestOffsets: Uint32Array;
  pkOffsets?: Uint32Array;
  pubkeys?: Uint8Array;
  pubkeyIndices?: Uint32Array;
  messages: Uint8Array;
  signatures: Uint8Array;
  sigOffsets: Uint32Array;
  seed: Uint8Array;
  batchable?: Uint8Array;
  /** keys by descriptor (lb_key_source), instead of pkOffsets / pubkeys / pubkeyIndices: five
   * words per set (lb_set_keys: kind, list, a, len, bitsOff), the SLICE sets' indices, the BITS
   * sets' bytes */
  setKeys?: Uint32Array;
  keyPool?: Uint32Array;
  keyBits?: Uint8Array;
};

export type SameMessageBatch = {
  jobOffsets: Uint32Array;
  pubkeys?: Uint8Array;
  pubkeyIndices?: Uint32Array;
  signatures: Uint8Array;
  sigOffsets: Uint32Array;
  messages: Uint8Array;
  seed: Uint8Array;
};

export type VerifyResult = {
  valid: Uint8Array;
  errors: Uint8Array;
  setStatus: Uint8Array;
  batchRetries: number;
  batchSigsSuccess: number;
  deviceMs: number;
  workerStartNs?: number;
  workerEndNs?: number;
};

/** One GPU: the N-API addon's Context (lodestar_amd/napi/addon.cc), or a mock. */
export interface GpuBackend {
  capacity?: number;
  /** the addon Context's same-message aggregation mode in force */
  readonly sameMessageRandomized?: boolean;
  verifyRequests(batch: PackedRequests, opts?: {priority?: boolean}): Promise<VerifyResult>;
  verifyRequestsPartial?(batch: PackedRequests): Promise<{id: number; partial: Uint8Array}>;
  finish?(id: number, mergedOk: boolean): Promise<VerifyResult>;
  gtCheck?(partials: Uint8Array): Promise<boolean>;
  /** opts.aggregate: the result also carries each job's aggregate signature (96 bytes each, the
   * compressed sum of its valid sets that opts.mask -- one byte per set -- keeps) and count */
  verifySameMessage(batch: SameMessageBatch, opts?: {aggregate?: boolean; mask?: Uint8Array}): Promise<{
    valid: Uint8Array;
    jobFast: Uint8Array;
    retriedJobs: number;
    fastSets: number;
    deviceMs: number;
    jobSignatures?: Uint8Array;
    jobCounts?: Uint32Array;
  }>;
  aggregateSignatureGroups?(
    batch: {groupOffsets: Uint32Array; signatures: Uint8Array; sigOffsets: Uint32Array},
    opts?: {noCheck?: boolean}
  ): Promise<{signatures: Uint8Array; badIndex: Int32Array}>;
  syncPubkeys?(keys: Uint8Array, pkLen: number): Promise<number>;
  /** lb_index_list_put: resolves to the list's size */
  indexListPut?(listId: number, indices: Uint32Array): Promise<number>;
  /** lb_index_list_shuffle: resolves to unshuffleList(activeIndices, seed), which list `listId` now holds */
  indexListShuffle?(listId: number, activeIndices: Uint32Array, seed: Uint8Array): Promise<Uint32Array>;
  /** lb_balance_table_put: resolves to the balance table's size */
  balanceTablePut?(first: number, increments: Uint8Array): Promise<number>;
  /** lb_sample_by_balance (seeds: 32 bytes each); indices: seeds x count, 0xFFFFFFFF where unfilled.
   * storeList: a lone seed's filled result replaces that index list on the device; with aggregate,
   * aggregatePubkey is lb_aggregate_pubkeys_list of the stored list (96 bytes) */
  sampleByBalance?(req: {
    seeds: Uint8Array;
    count: number;
    activeIndices: Uint32Array;
    maxIncrement: number;
    maxCandidates: number;
    storeList?: number;
    aggregate?: boolean;
  }): Promise<{indices: Uint32Array; found: Uint32Array; tried: Uint32Array; aggregatePubkey?: Uint8Array}>;
  aggregatePubkeys?(keys: Uint8Array | Uint32Array): Promise<Uint8Array>;
  /** KZG_SETUP_G2_MONOMIAL[1], 96 bytes compressed; a refused point rejects and keeps the old setup */
  kzgLoadSetup?(g2Tau: Uint8Array): Promise<void>;
  /** blobs n x 131072, commitments and proofs n x 48 bytes (n <= 64); status: 0 OK, 1 BAD_BLOB,
   * 2 BAD_COMMITMENT, 3 BAD_PROOF, 4 BAD_SCALAR -- what c-kzg throws on; ok is false when any is set */
  kzgVerifyBlobProofBatch?(
    blobs: Uint8Array,
    commitments: Uint8Array,
    proofs: Uint8Array
  ): Promise<{ok: boolean; status: Uint8Array}>;
  /** the 4096 G1 Lagrange lines of trusted_setup.txt (48 bytes each, file order); a refused point
   * rejects with its index in the message and keeps the old table */
  kzgLoadSetupG1?(g1Lagrange: Uint8Array): Promise<void>;
  /** blobToKzgCommitment / computeBlobKzgProof / computeKzgProof of n <= 64 items; an item with a
   * status has all-zero outputs, the others are computed */
  kzgBlobCommitments?(blobs: Uint8Array): Promise<{commitments: Uint8Array; status: Uint8Array}>;
  kzgBlobProofs?(blobs: Uint8Array, commitments: Uint8Array): Promise<{proofs: Uint8Array; status: Uint8Array}>;
  kzgComputeProofs?(blobs: Uint8Array, zs: Uint8Array): Promise<{proofs: Uint8Array; ys: Uint8Array; status: Uint8Array}>;
  close?(): Promise<void>;
}

/** The blob methods of `ckzg` (BN/util/kzg.ts:15-22) on the GPU (kzg.js).  Throws where c-kzg
 * throws (lengths, a field element >= r, bytes that are no G1 point), false only for a failed
 * pairing check.  Every method but freeTrustedSetup returns a Promise: the addon never blocks the
 * event loop.  On a backend without kzgBlobCommitments / kzgBlobProofs the two compute methods
 * throw "not implemented: use c-kzg" synchronously. */
export interface GpuKzg {
  freeTrustedSetup(): void;
  loadTrustedSetup(filePath: string): Promise<void>;
  blobToKzgCommitment(blob: Uint8Array): Promise<Uint8Array>;
  computeBlobKzgProof(blob: Uint8Array, commitment: Uint8Array): Promise<Uint8Array>;
  blobsToKzgCommitments(blobs: Uint8Array[]): Promise<Uint8Array[]>;
  computeBlobKzgProofs(blobs: Uint8Array[], commitments: Uint8Array[]): Promise<Uint8Array[]>;
  /** -> [proof, y] */
  computeKzgProof(blob: Uint8Array, z: Uint8Array): Promise<[Uint8Array, Uint8Array]>;
  verifyBlobKzgProof(blob: Uint8Array, commitment: Uint8Array, proof: Uint8Array): Promise<boolean>;
  verifyBlobKzgProofBatch(
    blobs: Uint8Array[],
    expectedKzgCommitments: Uint8Array[],
    kzgProofs: Uint8Array[]
  ): Promise<boolean>;
}
export function createGpuKzg(backend: GpuBackend): GpuKzg;
export function parseTrustedSetupG1(text: string): Uint8Array;

/** verifyAndAggregateSameMessage: the verdicts, and what attestationPool.add would have built from
 * the valid signatures -- their 96-byte compressed sum (null when count is 0) and how many. */
export type SameMessageAggregate = {valid: boolean[]; signature: Uint8Array | null; count: number};

export type BlsGpuVerifierOpts = {
  /** GPU ordinals, one addon Context each (default [0]) */
  devices?: number[];
  /** Context-like objects instead (tests: mocks) */
  backends?: GpuBackend[];
  /** calls in flight per GPU (default: the library's lb_slots) */
  capacity?: number;
  blsVerifyAllMultiThread?: boolean;
  maxSetsPerDispatch?: number;
  prefetch?: number;
  seedSource?: () => Uint8Array;
  /** priority jobs and verifyOnMainThread calls take the device's priority lane (default true) */
  priorityLane?: boolean;
  /** same-message jobs aggregated with per-set random 64-bit scalars (LB_SM_RANDOMIZED: a passing
   * aggregate implies every set valid) instead of plain sums; applies to the contexts created
   * here, their latency lanes included (default false: the library's initial mode) */
  sameMessageRandomized?: boolean;
  /** the addon module the contexts are created from (tests: a stand-in; default loadAddon()) */
  addon?: AddonModule;
};

/** BlsMultiThreadWorkerPool (chain/bls/multithread/index.ts) on GPUs. */
export class BlsGpuVerifier implements IBlsVerifier {
  constructor(opts?: BlsGpuVerifierOpts);
  readonly capacity: number;
  readonly metrics: PoolMetrics;
  /** Append keys to every GPU's pubkey table (pubkeyCache.ts:56-77); PublicKey objects are
   * serialized once here and then ship as their table index.  Returns the table size. */
  syncPubkeys(keys: (Uint8Array | PublicKeyLike)[], pkLen?: 48 | 96): Promise<number>;
  /** computeEpochShuffling's unshuffleList on the GPU (8 list ids, 0..7): every GPU keeps the
   * shuffling as index list `listId`; resolves to it for the node's EpochShuffling */
  syncShuffling(listId: number, activeIndices: Uint32Array | number[], seed: Uint8Array): Promise<Uint32Array>;
  /** indices as given (a sync committee's 512) as index list `listId` */
  putIndexList(listId: number, indices: Uint32Array | number[]): Promise<void>;
  /** EffectiveBalanceIncrements to every GPU's balance table, from validator index `first`; the table's size */
  syncBalances(increments: Uint8Array | number[], first?: number): Promise<number>;
  /** computeProposers (util/seed.ts:22-80) on the GPU; -1 where a slot found no proposer */
  computeProposers(
    epochSeed: Uint8Array,
    startSlot: number,
    activeIndices: Uint32Array | number[],
    slots?: number,
    maxIncrement?: number
  ): Promise<number[]>;
  /** getNextSyncCommitteeIndices + aggregatePubkey on the GPU; the committee becomes index list `listId` */
  syncCommittee(
    listId: number,
    activeIndices: Uint32Array | number[],
    seed: Uint8Array,
    size?: number,
    maxIncrement?: number,
    maxCandidates?: number
  ): Promise<{indices: Uint32Array; aggregatePubkey: Uint8Array}>;
  /** pubkeyCache.syncPubkeys for the GPUs: mirror index2pubkey's new entries (incremental);
   * returns the number of entries mirrored. */
  syncIndex2pubkey(index2pubkey: PublicKeyLike[]): Promise<number>;
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  verifySignatureSetsSameMessage(
    sets: {publicKey: GpuPublicKey; signature: Uint8Array}[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<boolean[]>;
  /** One job of any size; opts.include[i] === false leaves set i out of the sum only.  In the plain
   * mode a fast-path job may hold a cancelling pair: sum subsets under sameMessageRandomized. */
  verifyAndAggregateSameMessage(
    sets: {publicKey: GpuPublicKey; signature: Uint8Array}[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread"> & {include?: boolean[]}
  ): Promise<SameMessageAggregate>;
  /** bls.Signature.aggregate(group).toBytes() per group in one device call; throws on an empty
   * group or a signature that fails to load (noCheck: signatureFromBytesNoCheck) */
  aggregateSignatureGroups(groups: Uint8Array[][], opts?: {noCheck?: boolean}): Promise<Uint8Array[]>;
  close(): Promise<void>;
  canAcceptWork(): boolean;
}

/** BlsSingleThreadVerifier (chain/bls/singleThread.ts:10-89) on one GPU. */
export class BlsGpuSingleThreadVerifier implements IBlsVerifier {
  constructor(opts?: {
    backend?: GpuBackend;
    device?: number;
    seedSource?: () => Uint8Array;
    metrics?: PoolMetrics;
    /** as BlsGpuVerifierOpts.sameMessageRandomized, for the context created here */
    sameMessageRandomized?: boolean;
    addon?: AddonModule;
  });
  syncPubkeys(keys: (Uint8Array | PublicKeyLike)[], pkLen?: 48 | 96): Promise<number>;
  /** computeEpochShuffling's unshuffleList on the GPU (8 list ids, 0..7): every GPU keeps the
   * shuffling as index list `listId`; resolves to it for the node's EpochShuffling */
  syncShuffling(listId: number, activeIndices: Uint32Array | number[], seed: Uint8Array): Promise<Uint32Array>;
  /** indices as given (a sync committee's 512) as index list `listId` */
  putIndexList(listId: number, indices: Uint32Array | number[]): Promise<void>;
  /** EffectiveBalanceIncrements to every GPU's balance table, from validator index `first`; the table's size */
  syncBalances(increments: Uint8Array | number[], first?: number): Promise<number>;
  /** computeProposers (util/seed.ts:22-80) on the GPU; -1 where a slot found no proposer */
  computeProposers(
    epochSeed: Uint8Array,
    startSlot: number,
    activeIndices: Uint32Array | number[],
    slots?: number,
    maxIncrement?: number
  ): Promise<number[]>;
  /** getNextSyncCommitteeIndices + aggregatePubkey on the GPU; the committee becomes index list `listId` */
  syncCommittee(
    listId: number,
    activeIndices: Uint32Array | number[],
    seed: Uint8Array,
    size?: number,
    maxIncrement?: number,
    maxCandidates?: number
  ): Promise<{indices: Uint32Array; aggregatePubkey: Uint8Array}>;
  syncIndex2pubkey(index2pubkey: PublicKeyLike[]): Promise<number>;
  verifySignatureSets(sets: ISignatureSet[]): Promise<boolean>;
  verifySignatureSetsSameMessage(
    sets: {publicKey: GpuPublicKey; signature: Uint8Array}[],
    message: Uint8Array
  ): Promise<boolean[]>;
  verifyAndAggregateSameMessage(
    sets: {publicKey: GpuPublicKey; signature: Uint8Array}[],
    message: Uint8Array,
    opts?: {include?: boolean[]}
  ): Promise<SameMessageAggregate>;
  aggregateSignatureGroups(groups: Uint8Array[][], opts?: {noCheck?: boolean}): Promise<Uint8Array[]>;
  close(): Promise<void>;
  canAcceptWork(): boolean;
}

export const QueueErrorCode: {QUEUE_ABORTED: "QUEUE_ERROR_QUEUE_ABORTED"};
export class QueueError extends Error {
  constructor(code: string);
  type: {code: string};
}

/** The reference's metric names (metrics/metrics/lodestar.ts:379-510), kept in-process. */
export class PoolMetrics {
  inc(name: string, v?: number, labels?: Record<string, string | number>): void;
  set(name: string, v: number, labels?: Record<string, string | number>): void;
  observe(name: string, v: number, labels?: Record<string, string | number>): void;
  get(name: string, labels?: Record<string, string | number>): number;
}
export const METRICS: Record<string, string>;

export function chunkifyMaximizeChunkSize<T>(arr: T[], minPerChunk: number): T[][];
export function workerBatchStats(
  requestSizes: number[],
  batchable: boolean[],
  valid: boolean[]
): {retries: number; sigsOk: number};
export function packRequests(
  requests: ISignatureSet[][],
  seed: Uint8Array,
  keyMap?: WeakMap<object, number>
): PackedRequests;
export function packSameMessage(
  jobs: {sets: {publicKey: GpuPublicKey; signature: Uint8Array}[]; message: Uint8Array}[],
  seed: Uint8Array,
  keyMap?: WeakMap<object, number>
): SameMessageBatch;
export function shardRequests(sizes: number[], nShards: number): [number, number][];
export function slicePacked(p: PackedRequests, lo: number, hi: number, seed: Uint8Array): PackedRequests;
/** Several GPUs, one combined final exponentiation over the shards' Fp12 partials. */
export function verifyRequestsSharded(
  backends: GpuBackend[],
  requests: ISignatureSet[][],
  seedSource: () => Uint8Array
): Promise<{valid: Uint8Array; errors: Uint8Array; mergedOk: boolean}>;
export function verifyPackedSharded(
  backends: GpuBackend[],
  packed: PackedRequests,
  seedSource: () => Uint8Array
): Promise<{valid: Uint8Array; errors: Uint8Array; mergedOk: boolean}>;
export type AddonModule = {
  deviceCount?(): number;
  Context: new (device: number, opts?: {capacity?: number; sameMessageRandomized?: boolean}) => GpuBackend;
};
export function loadAddon(): AddonModule;

export const MAX_SIGNATURE_SETS_PER_JOB: 128;
export const MAX_BUFFERED_SIGS: 32;
export const MAX_BUFFER_WAIT_MS: 100;
export const MAX_JOBS_CAN_ACCEPT_WORK: 512;
export const MAX_PRIORITY_LANE_SETS: 1024;
/** lb_request_batch / lb_same_message_batch pubkeyIndices flags (include/lodestar_bls.h) */
export const LB_PK_ROW_FLAG: 0x80000000;
export const LB_PK_ROW48_FLAG: 0x40000000;
