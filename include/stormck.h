/*
 * stormck — MI355X-native block-checksum engine for storm (C ABI).
 *
 * Drop-in boundary for storm's per-block content hash (Go package `blocks`):
 *
 *   func Checksum(b []byte) Hash                         /root/reference/blocks/checksum.go:15-17
 *   func BlockChecksum[T Block](b *T) Hash               /root/reference/blocks/checksum.go:10-12
 *   func VerifyChecksum(address, p, expected) error      /root/reference/blocks/checksum.go:20-27
 *   type Pointer struct{Checksum, Address, BirthRevision} /root/reference/blocks/types.go:35-39
 *
 * The hash is XXH64 with seed 0 (github.com/cespare/xxhash/v2 v2.2.0 Sum64,
 * /root/reference/go.mod:6), bit-exact. All entry points are plain C: pointers and
 * sizes only. Every function returns 0 on success or a negative STORMCK_E* code;
 * stormck_last_error() then holds a thread-local message.
 *
 * "_device" entry points take device pointers (HBM) and a hipStream_t passed as
 * void* (NULL = the null stream of the calling thread's current device); they are
 * asynchronous with respect to the host, like any kernel launch on that stream.
 * "_host" entry points take host memory and return when the results are in host
 * memory (H2D -> kernel -> D2H, pipelined).
 *
 * There is no CPU fallback: without a usable gfx950 device every batched, device,
 * routed and Merkle entry point returns STORMCK_ENODEV. Host computation is a measured leg,
 * never a substitute for a missing device:
 *  - the latency leg of a SINGLE call (stormck_xxh64 / stormck_checksum): one buffer is
 *    four serial XXH64 chains, which one host core walks faster than the GPU at every
 *    length, so single calls stay on the host by design;
 *  - the host legs of data that lives in HOST memory (stormck_commit_host,
 *    stormck_checksum_host_leg), which the routed entry points (stormck_commit,
 *    stormck_checksum_batch) run alone, or beside the devices (the split leg), when the
 *    library's cost model predicts that is faster than the PCIe-bound device leg.
 */
#ifndef STORMCK_H
#define STORMCK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STORMCK_ABI_VERSION 7

#define STORMCK_OK 0
#define STORMCK_EINVAL (-1)  /* bad argument (null pointer, n/len/stride out of range, ...) */
#define STORMCK_EHIP (-2)    /* HIP runtime error */
#define STORMCK_ENODEV (-3)  /* no usable gfx950 device */
#define STORMCK_ENOMEM (-4)  /* device / pinned allocation failed */
#define STORMCK_EMISMATCH (-5) /* verify: at least one checksum differs (see first_bad) */

/* storm block types, blocks/types.go:7-15 */
#define STORMCK_FREE_BLOCK 0
#define STORMCK_POINTER_BLOCK 1
#define STORMCK_LEAF_BLOCK 2

/* storm's PointersPerBlock (blocks/pointer/params.go:6; 10 under the `test` build tag,
 * blocks/pointer/params_testing.go:6). */
#define STORMCK_POINTERS_PER_BLOCK 1200

/* blocks.Pointer, 24 bytes, Go amd64 layout (blocks/types.go:35-39). */
typedef struct stormck_pointer {
    uint64_t checksum;
    uint64_t address;
    uint64_t birth_revision;
} stormck_pointer;

/* ---- library / device ---------------------------------------------------- */

int stormck_abi_version(void);
/* Provenance of this build: "sha256:<hex>" of the sources it was compiled from
 * (storm_amd/build.py SOURCES), so a prebuilt library can be matched to a tree. */
const char* stormck_build_id(void);
const char* stormck_last_error(void);
/* Number of visible gfx950 devices (0 on a machine without one). */
int stormck_device_count(int* count);
/* Select `device` for the calling thread and register its context. Pinned staging
 * for the host path is allocated lazily by the first _host call on that device. */
int stormck_init(int device);
/* Free pinned staging / device buffers of every context. */
void stormck_shutdown(void);
/* Ring-kernel faults. The small-batch kernels stage blocks through an LDS ring whose
 * waits are bounded; a wait that expires (a liveness bug, never expected) is an error,
 * not a value: the kernel writes no checksum for the blocks of the stalled workgroup (a
 * verify counts each of them as a mismatch, so it fails closed) and records the fault in
 * the slot of the STREAM it was launched on. Host-synchronous entry points (_host,
 * _host_multi, stormck_commit_device, stormck_read_verify_fd) check their own streams'
 * slots after their sync and return STORMCK_EHIP naming the kernel; their outputs are
 * then unspecified. For the asynchronous _device entry points, stormck_device_status
 * synchronises `stream` and returns STORMCK_EHIP if a ring kernel launched on that
 * stream (on the calling thread's current device) faulted since the last check (the
 * fault is then cleared), otherwise the stream's own status. Faults never cross streams:
 * concurrent callers on distinct streams see only their own (the legacy null stream is
 * one stream, shared by every thread of the device). The slots are allocated by
 * stormck_init; a first ring launch inside a stream capture without it is STORMCK_EINVAL.
 * A ring launch captured into a graph reports into the slot of the stream it was
 * captured on, so check that stream after replays (status on a stream that is being
 * captured is STORMCK_EINVAL).
 * Up to 1024 streams per device have a slot of their own at once; past that the least
 * recently launched stream with no pending fault gives its slot up. */
int stormck_device_status(void* stream);
/* Release `stream`'s fault slot on the calling thread's current device; call it before
 * destroying a stream that ring kernels were launched on. It synchronises the stream, and
 * returns STORMCK_EHIP if a fault was still pending there (which is then cleared), so a
 * stream created later with the same handle never inherits it. */
int stormck_stream_forget(void* stream);
/* Device memory for a block arena (storm's cache.data mirrored in HBM): hipMalloc on the
 * calling thread's current device, outside any caching allocator, so an arena taken first
 * in a process is placed the same way whatever else the process allocates. */
int stormck_device_alloc(uint64_t bytes, void** d_ptr);
int stormck_device_free(void* d_ptr);

/* ---- hot path: batch checksums of device-resident blocks -------------------
 * Block i starts at d_base + i*stride and is (d_lens ? d_lens[i] : len) bytes
 * long. out[i] = XXH64(block i) = blocks.Checksum(block bytes). Any alignment is
 * accepted; 8-byte-aligned blocks take the fast path. n == 0 is a no-op.
 * With d_lens, len may carry an upper bound of the lengths (0 = unknown), which the
 * library plans the launch with: batches of short blocks (storm's `-tags test` sizes)
 * take a different kernel than 32 KiB ones. Results never depend on it. The same holds
 * for the gather and verify entry points below. */
int stormck_checksum_device(const void* d_base, uint64_t stride, const uint32_t* d_lens, uint32_t len,
                            uint64_t n, uint64_t* d_out, void* stream);

/* Same, block i at d_base + d_offsets[i] (e.g. the dirty slots of storm's cache.data,
 * /root/reference/cache/cache.go:36-40). */
int stormck_checksum_gather_device(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                                   uint32_t len, uint64_t n, uint64_t* d_out, void* stream);

/* Batched blocks.VerifyChecksum. d_result[0] = index of the first block whose checksum
 * differs from d_expected (n if none), d_result[1] = number of mismatches. The result
 * is written on `stream` (no host sync); check it after synchronising. */
int stormck_verify_device(const void* d_base, uint64_t stride, const uint32_t* d_lens, uint32_t len,
                          uint64_t n, const uint64_t* d_expected, uint64_t* d_result, void* stream);

/* ---- host-memory batch (starts and ends in host memory) -------------------- */

/* out[i] = XXH64 of host block i (base + i*stride, lens ? lens[i] : len). Pipelined
 * H2D / kernel / D2H through library-owned pinned staging on the calling thread's
 * current device; memory registered with stormck_host_register is DMA'd directly. */
int stormck_checksum_host(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                          uint64_t* out);
/* Batched verify of host blocks: *first_bad = first mismatching index (n if none),
 * *n_bad = mismatch count. Returns STORMCK_EMISMATCH if n_bad > 0. */
int stormck_verify_host(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                        const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad);
/* The same two calls spread over several devices from one process (storm is one Go
 * process; each device has its own PCIe link): the n blocks split into n_devices
 * contiguous ranges whose sizes differ by at most one, and range k runs on
 * devices[k] in its own host thread. Results are as from the single-device calls
 * (first_bad is the lowest mismatching index of the whole batch, n_bad the total).
 * A device may be listed more than once; its ranges then run one after another.
 * Memory registered with stormck_host_register is pinned for every device. The
 * calling thread's current device is left as it was. On failure the message names
 * the device and block range of the lowest failing range. */
int stormck_checksum_host_multi(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                                uint64_t* out, const int* devices, int n_devices);
int stormck_verify_host_multi(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                              const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, const int* devices,
                              int n_devices);
/* A host-memory batch routed by cost (the Go shim's ChecksumBatch / VerifyChecksumBatch).
 * Over PCIe a device moves about 52 GiB/s end to end, while host threads hash the same
 * bytes four blocks at a time (AVX-512) until host memory binds: stormck_checksum_batch runs
 * each batch on the leg the library's cost model predicts is fastest (the routing section
 * below): the host leg, the device leg (stormck_checksum_host, or _host_multi over the route
 * devices), or, for pinned or registered memory, the split leg (both at once).
 * host_threads: threads the host part may use (0 = the library pool, at most 16; 1 = keep
 * the other cores for the caller; a call that finds the pool held by another call plans
 * with its own thread only). *leg_used (optional) = STORMCK_LEG_HOST / _DEVICE / _SPLIT.
 * Same arguments, results and errors as the _host calls; device memory, or memory the host
 * cannot read, is STORMCK_EINVAL (use _device). Needs a gfx950 device like every batched
 * entry point: STORMCK_ENODEV without one, even when the model would pick the host leg
 * (a stormck build needs its GPU).
 * stormck_checksum_host_leg / stormck_verify_host_leg: the host leg alone, on `threads`
 * pool threads (0 = the pool); needs no device. */
int stormck_checksum_batch(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                           uint64_t* out, uint32_t host_threads, uint32_t* leg_used);
int stormck_verify_batch(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                         const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, uint32_t host_threads,
                         uint32_t* leg_used);
int stormck_checksum_host_leg(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                              uint64_t* out, uint32_t threads);
int stormck_verify_host_leg(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                            const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, uint32_t threads);
/* ---- single calls (Go blocks.Checksum / BlockChecksum / VerifyChecksum, one block)
 * stormck_xxh64: XXH64 seed 0 of p[0..n_bytes) on the calling host thread; cannot
 * fail (p may be NULL only when n_bytes == 0). What the Go shim's Checksum calls.
 * stormck_checksum: the single-call dispatch. Below the measured host/device crossover
 * (never reached: the device single call is slower at every length, DESIGN_LOG.md §5) it
 * is stormck_xxh64; any length, no device needed.
 * stormck_checksum_gpu: the same hash through the device: one k_xxh64_single launch
 * for slices up to 64 KiB, the host pipeline with a batch of one up to 256 MiB;
 * longer slices return STORMCK_EINVAL. Needs a device. */
uint64_t stormck_xxh64(const void* p, uint64_t n_bytes);
int stormck_checksum(const void* p, uint64_t n_bytes, uint64_t* out);
int stormck_checksum_gpu(const void* p, uint64_t n_bytes, uint64_t* out);
/* Page-lock and map a host range (for every device) so the device and split legs DMA it or
 * read it in place, without staging copies. Also sets up the calling thread's current
 * device's staging for those legs (once per process: 2.25 GiB of HBM and 1 GiB of pinned
 * host memory, ~0.3 s), so the first routed call that uses the device does not pay for it.
 * The library keeps the range in its own list (the routed calls recognise it without a
 * runtime query): release it with stormck_host_unregister, not hipHostUnregister directly. */
int stormck_host_register(void* p, uint64_t bytes);
int stormck_host_unregister(void* p);
/* Device-visible address of host memory registered with stormck_host_register: the
 * *_device entry points (stormck_commit_device's arena included) then read and write
 * it in place over PCIe. This runs f1 on storm's cache.data where it lives, in host
 * memory (cache/cache.go:36-40), at link rate instead of HBM rate. Block rows must be
 * 256-byte aligned for that (a 16-byte offset costs about a quarter of the rate). */
int stormck_host_device_pointer(void* p, void** d_p);

/* ---- Merkle pointer tree (storm pointer.Block nodes) -----------------------
 * One level: children are entries {cs[i], child_addr_base + i, rev}, all of type
 * child_type. Parent j packs children [j*fanout, min((j+1)*fanout, m)) into a storm
 * pointer.Block (blocks/pointer/block.go:10-13; size = 25*fanout rounded up to 8
 * bytes, unused slots zero) and d_parent_cs[j] = XXH64(that block). The node bytes
 * are never materialised: each word is synthesised from the child arrays. */
int stormck_pointer_level_device(const uint64_t* d_child_cs, uint64_t m, uint64_t child_addr_base,
                                 uint64_t rev, uint8_t child_type, uint32_t fanout, uint64_t* d_parent_cs,
                                 void* stream);
/* One node from explicit entries (d_entries[0..count), d_types[0..count)), count <=
 * fanout. Writes *d_out_cs. Used to combine per-shard roots. */
int stormck_pointer_node_device(const stormck_pointer* d_entries, const uint8_t* d_types, uint32_t count,
                                uint32_t fanout, uint64_t* d_out_cs, void* stream);
/* Materialise pointer blocks of one level (same rule as pointer_level) into
 * d_blocks (pm blocks at dst_stride bytes), e.g. to be written to storage. */
int stormck_pack_pointer_blocks_device(const uint64_t* d_child_cs, uint64_t m, uint64_t child_addr_base,
                                       uint64_t rev, uint8_t child_type, uint32_t fanout, void* d_blocks,
                                       uint64_t dst_stride, void* stream);
/* Workspace bytes stormck_merkle_root_device needs for n leaves. */
uint64_t stormck_merkle_workspace_bytes(uint64_t n, uint32_t fanout);
/* Whole shard tree (DESIGN.md "Shard Merkle tree"): leaves {d_leaf_cs[i],
 * leaf_addr_base + i, rev} of type Leaf; interior nodes get addresses
 * node_addr_base, node_addr_base+1, ... level by level, bottom-up. Writes the root
 * Pointer to *d_root and its type to *d_root_type (device memory). n == 0 -> zero root,
 * type Free; n == 1 -> the leaf's own pointer, type Leaf. */
int stormck_merkle_root_device(const uint64_t* d_leaf_cs, uint64_t n, uint64_t leaf_addr_base,
                               uint64_t node_addr_base, uint64_t rev, uint32_t fanout, void* d_workspace,
                               uint64_t workspace_bytes, stormck_pointer* d_root, uint8_t* d_root_type,
                               void* stream);

/* ---- multi-GPU, one process: device-resident shards and their global root (c4) --------
 * storm is one Go process; on an 8-GPU node it reaches every GPU from it.
 * A batch of device-resident blocks is sharded into contiguous ranges, each on its own
 * device. stormck_merkle_root_multi runs each shard's checksums (optional) and its shard
 * tree (stormck_merkle_root_device) on the shard's device, from one host thread per device,
 * gathers the shard roots over xGMI with in-process RCCL (ncclCommInitAll over the distinct
 * devices, one ncclAllGather of their root rows), and hashes the combining pointer block on
 * EVERY device; the devices must agree. The reference has no multi-device code; the tree
 * shape is this library's and the node format storm's (blocks/pointer/block.go:10-13).
 * One shard: */
typedef struct stormck_shard {
    const void* d_blocks;    /* block i at d_blocks + i*stride on `device`, `len` bytes; NULL: the
                              * leaf checksums are already in d_checksums (nothing is hashed) */
    uint64_t stride;
    uint64_t n;              /* leaves of the shard */
    uint64_t* d_checksums;   /* n u64 on `device`: written when d_blocks is set, else read */
    uint64_t leaf_addr_base; /* Address of leaf i is leaf_addr_base + i (Leaf type, rev) */
    uint64_t node_addr_base; /* interior nodes: node_addr_base, +1, ... level by level, bottom-up */
    void* stream;            /* a stream of `device` the shard's work runs on, after what is already
                              * queued there (e.g. the launches that wrote d_checksums); NULL: the
                              * library's own stream, which waits for no other stream. A stream of
                              * another device is STORMCK_EINVAL */
    int32_t device;          /* HIP device index holding the shard */
    uint32_t len;            /* bytes hashed per block (when d_blocks is set) */
} stormck_shard;

/* The build's shard convention (storm_amd/dist.py): n_total leaves in n_shards
 * contiguous ranges whose sizes differ by at most one; shard s holds leaves [lo_s, hi_s),
 * addressed lo_s..hi_s-1, its interior nodes from n_total + lo_s (disjoint from every other
 * shard's and from the leaves for fanout >= 3), and the combining node gets 2 * n_total.
 * Fills n, leaf_addr_base, node_addr_base and device (shards are dealt to devices[0..n_devices)
 * in consecutive runs: shard s on devices[s * n_devices / n_shards]) of shards[0..n_shards) and
 * zeroes the rest; the caller sets d_blocks / stride / len / d_checksums / stream, with shard
 * s's blocks being logical blocks [lo_s, hi_s) (lo_s = leaf_addr_base). *root_addr (optional)
 * = 2 * n_total. Needs no device. */
int stormck_shard_plan(uint64_t n_total, uint32_t n_shards, const int* devices, int n_devices, stormck_shard* shards,
                       uint64_t* root_addr);

/* The global root of shards[0..n_shards) (1 <= n_shards <= fanout): every shard's tree
 * (leaves of type Leaf, birth revision rev), then one pointer block holding the shard roots
 * in shard order, hashed on every device: *root = {its checksum, root_addr, rev}, *root_type =
 * Pointer. shard_roots / shard_types (optional, n_shards each) = the shard roots (a shard of
 * n == 0 has a zero root of type Free, of n == 1 its leaf's own Pointer). Synchronous: returns
 * when every shard's work and the gather have finished; the shards' streams may then be reused.
 * A device may hold several shards (the gather then carries several rows per device; with one
 * device the gather is a one-rank RCCL communicator). RCCL (librccl.so.1, from the ROCm
 * install or already in the process) is loaded at the first call and its communicators are
 * kept per device set; STORMCK_EHIP names an RCCL that cannot be loaded or fails. Calls are
 * serialised process-wide (a communicator serves one collective at a time). */
int stormck_merkle_root_multi(const stormck_shard* shards, uint32_t n_shards, uint64_t rev, uint64_t root_addr,
                              uint32_t fanout, stormck_pointer* root, uint8_t* root_type, stormck_pointer* shard_roots,
                              uint8_t* shard_types);

/* The gather layout stormck_merkle_root_multi uses for shards[0..n_shards), without a device
 * (planning only; device indices are not checked against the visible devices):
 * devices[0..*n_devices) = the shards' distinct devices in order of first appearance (the
 * communicator's ranks), *rows = R, the most shards on one device (each device sends R root
 * rows of 32 bytes; rows it does not fill stay zero), table_row[s] = the row of the gathered
 * D x R table holding shard s's root (device slot * R + the shard's place among that device's
 * shards). devices needs room for 64 entries. */
int stormck_multi_layout(const stormck_shard* shards, uint32_t n_shards, int32_t* devices, uint32_t* n_devices,
                         uint32_t* rows, uint32_t* table_row);

/* ---- f2/f3: batched cold read + verify from a file device -------------------
 * storm's cold fetch reads a block from its Dev and verifies it
 * (cache.fetchBlock: Store.ReadBlock(address, Data[:Sizeof(T)]) then
 * blocks.VerifyChecksum, /root/reference/cache/cache.go:139-167,
 * persistence/store.go:39-51; filedev = *os.File, pkg/filedev/filedev.go). This
 * does it for n blocks at once: block i (lens[i] bytes at file offset
 * addresses[i] * block_size) is read with parallel pread() into
 * dst + i*dst_stride (e.g. the cache slots), then all n are verified on the GPU
 * against expected[i]. With STORMCK_READ_FULL_BLOCK each read covers block_size
 * bytes while lens[i] bytes are still what is hashed. A descriptor opened with
 * O_DIRECT (no page cache) always reads full blocks; dst, dst_stride and block_size
 * must then be 512-byte aligned (the device's own alignment may be stricter).
 * Consecutive addresses whose slots are contiguous (dst_stride == block_size) are
 * read with one pread of up to 1 MiB. With dst registered (stormck_host_register)
 * the verify DMAs straight from the slots, with no staging copy.
 * *first_bad = first mismatching index (n if none), *n_bad = count; returns
 * STORMCK_EMISMATCH if any block fails, STORMCK_EINVAL on a short read. */
#define STORMCK_READ_FULL_BLOCK 1u
int stormck_read_verify_fd(int fd, const uint64_t* addresses, const uint32_t* lens, uint64_t n, uint64_t block_size,
                           void* dst, uint64_t dst_stride, const uint64_t* expected, uint32_t flags,
                           uint64_t* first_bad, uint64_t* n_bad);

/* ---- f4: key tags ----------------------------------------------------------
 * xxhash.Sum64(key) for a batch of short keys (keystore.GetObjectID /
 * EnsureObjectID hash each key to a tree tag: /root/reference/keystore/keystore.go:33,66;
 * keys are 1..256 bytes, objectlist.MaxKeyComponentLength). Key i is at
 * d_keys + (d_offsets ? d_offsets[i] : i*stride), (d_lens ? d_lens[i] : len) bytes;
 * any alignment. One lane per key. Same results as stormck_checksum_device, which
 * remains correct for keys of any length. */
int stormck_key_tags_device(const void* d_keys, uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens,
                            uint32_t len, uint64_t n, uint64_t* d_out, void* stream);

/* ---- f1: level-synchronous batched commit ----------------------------------
 * storm's Cache.Commit hashes dirty blocks children-first, one at a time
 * (commitData / commitBlock, /root/reference/cache/cache.go:87-137) and each
 * block's PostCommitFunc stores {Checksum, Address, BirthRevision} and its type
 * into the parent through a BlockOrigin (/root/reference/cache/trace.go:274-320,
 * cache/types.go BlockOrigin). Blocks at the same height are independent, so the
 * library commits a whole dirty forest one LEVEL per launch: hash every block of
 * the level (gather), then scatter its Pointer and type into its origin.
 *
 * One entry per dirty block (blockMetadata + BlockOrigin), offsets relative to the
 * device arena (storm's cache.data): */
#define STORMCK_NO_ORIGIN UINT64_MAX
#define STORMCK_NO_PARENT (-1)
typedef struct stormck_dirty_block {
    uint64_t data_offset;    /* block bytes: d_arena + data_offset (blockMetadata.Data) */
    uint64_t origin_pointer; /* arena offset of the blocks.Pointer the parent keeps for this block
                              * (BlockOrigin.Pointer; 8-byte aligned), or STORMCK_NO_ORIGIN */
    uint64_t origin_type;    /* arena offset of the parent's BlockType byte (BlockOrigin.BlockType) */
    int64_t parent;          /* index of the dirty block that holds the origin, or STORMCK_NO_PARENT
                              * (origin outside the batch, e.g. the singularity) */
    uint64_t address;        /* in/out: blockMetadata.Address */
    uint64_t birth_revision; /* in/out: blockMetadata.BirthRevision */
    uint32_t length;         /* bytes hashed = unsafe.Sizeof(T) */
    uint8_t type;            /* STORMCK_LEAF_BLOCK / STORMCK_POINTER_BLOCK, stored at origin_type */
    uint8_t reserved[3];
} stormck_dirty_block;

/* Commit the dirty forest blocks[0..n) held in d_arena:
 *  - order: children before parents (by height), index order within a height;
 *  - relocation, in that order (cache/cache.go:114-118): if birth_revision <=
 *    revision then address = ++*last_allocated_block, birth_revision = revision + 1;
 *  - per block: cs = XXH64(arena + data_offset, length); if origin_pointer is set,
 *    arena[origin_pointer] = Pointer{cs, address, birth_revision} and
 *    arena[origin_type] = type.
 * Writes out_checksums[i] (host) and updates blocks[i].address / birth_revision.
 * Synchronous on `stream`. Any children-first order is a valid storm commit order
 * (storm's own order follows Go map iteration); this one is deterministic.
 * Argument errors (parent range, origin alignment, cycles) and a missing device are
 * reported before anything is changed; of several defects every leg reports the one of the
 * lowest block whose check or walk to the root fails (any of them on several threads). A
 * HIP failure part-way leaves the commit partly applied, as storm's own loop does on a
 * write error; *last_allocated_block then still matches the relocations already written
 * into blocks. */
int stormck_commit_device(void* d_arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                          uint64_t* last_allocated_block, uint64_t* out_checksums, void* stream);

/* The same commit on host threads (the "host leg"): identical rules, order, relocation,
 * stores, outputs and errors as stormck_commit_device, with `arena` a HOST pointer
 * (storm's cache.data) and the blocks of one height hashed on `threads` library pool
 * threads (0 = all of the pool, at most 16; 1 = storm's serial loop). Needs no device:
 * it is the leg stormck_commit picks for forests too small to repay a launch per height
 * and the link (DESIGN_LOG.md §11 f1). */
int stormck_commit_host(void* arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                        uint64_t* last_allocated_block, uint64_t* out_checksums, uint32_t threads);
/* Cache.Commit's data phase as storm's cache calls it (the Go binding's CommitBatch):
 * `arena` is cache.data. An HBM arena (stormck_device_alloc) is committed by
 * stormck_commit_device. A host arena registered with stormck_host_register is committed
 * on the leg the library's cost model (routing section below) predicts is fastest: the
 * device leg in place over the link, the host leg on host_threads threads (0 = the pool),
 * or the split (stormck_commit_split: the leaves on both at once). An unregistered host
 * arena is out of the devices' reach and takes the host leg. Before a host or split leg
 * reads a registered arena, a non-NULL `stream` is synchronised (device writes the caller
 * queued on it land first). With `stream` NULL those legs wait for nothing: storm writes
 * cache.data on the host only (the Go binding passes nil), and the query would be most of
 * the routed call's cost on its smallest commits; a caller whose null-stream work writes the
 * arena synchronises it first (the device leg itself launches on the null stream then).
 * *leg_used (optional) = STORMCK_LEG_HOST / _DEVICE / _SPLIT. Needs a gfx950 device
 * like every batched entry point (STORMCK_ENODEV without one). */
#define STORMCK_LEG_NONE 0u
#define STORMCK_LEG_HOST 1u
#define STORMCK_LEG_DEVICE 2u
#define STORMCK_LEG_SPLIT 3u
int stormck_commit(void* arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                   uint64_t* last_allocated_block, uint64_t* out_checksums, void* stream, uint32_t host_threads,
                   uint32_t* leg_used);

/* ---- routing of host-memory work: the split leg and the measured rates -----------
 * Host-memory work (stormck_checksum_batch / _verify_batch, stormck_commit) runs on one of
 * three legs:
 *   STORMCK_LEG_HOST    the library's host threads alone;
 *   STORMCK_LEG_DEVICE  the device(s) alone, over PCIe;
 *   STORMCK_LEG_SPLIT   both at once on disjoint blocks of the one call: the host threads
 *                       take blocks from the front, each device takes chunks from the back,
 *                       each chunk sized from the rates so that the device finishes when the
 *                       host does, until they meet. The devices DMA (batch) or read in place
 *                       (commit) pinned or registered memory, with no host copy.
 * The choice is the smallest time a cost model predicts. Its rates (bytes per microsecond)
 * and the devices' start latency start at priors measured on an MI355X box and are measured
 * again by the calls themselves: every host, device or split leg large enough to time
 * updates its rate (EWMA). */
typedef struct stormck_route_rates {
    double host_thread;    /* one host thread (four blocks at once where the CPU has AVX-512) */
    double host_memory;    /* the host pool's cap on passes that stream from host memory */
    double host_cached;    /* the same on passes of at most 64 MiB, which can run from the host's
                            * caches (a commit hashes blocks its caller has just written) */
    double link_pinned;    /* one device's pipeline from pinned or registered host memory */
    double link_pageable;  /* one device's pipeline from pageable memory (through pinned staging) */
    double link_inplace;   /* one device's kernels reading registered host memory in place */
    double device_latency; /* microseconds from a split's start until a device's first chunk is
                            * back, beyond that chunk's bytes over the link (wake, launch, sync) */
    uint64_t observations; /* calls that updated the rates since the priors or the last set */
} stormck_route_rates;
int stormck_route_get_rates(stormck_route_rates* rates);
/* Replace the rates (rates == NULL: back to the priors). flags: STORMCK_RATES_FREEZE stops
 * the calls from updating them (tests, A/B); STORMCK_RATES_LEARN lets them. */
#define STORMCK_RATES_LEARN 0u
#define STORMCK_RATES_FREEZE 1u
int stormck_route_set_rates(const stormck_route_rates* rates, uint32_t flags);
/* The devices the routed entry points may use, process-wide (storm is one process; each
 * device brings its own PCIe link). n_devices == 0: the calling thread's current device
 * (the default). Listing a device twice lists it once. */
int stormck_route_devices(const int* devices, int n_devices);
/* The decision alone, from the model: no device and no data needed. memory:
 * STORMCK_MEM_PAGEABLE or STORMCK_MEM_PINNED (page-locked; for a commit, registered);
 * n_devices: devices the call could use (0: host leg only). *leg = the leg the routed call
 * would take (STORMCK_LEG_NONE for n == 0); predicted_us (optional, 3 doubles): host,
 * device and split time, INFINITY where the leg cannot run or the split gains nothing. A forest
 * that the commit's legs would refuse (stormck_commit_device) is STORMCK_EINVAL here too. */
#define STORMCK_MEM_PAGEABLE 0u
#define STORMCK_MEM_PINNED 1u
int stormck_route_plan_batch(uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n, uint32_t memory,
                             uint32_t host_threads, uint32_t n_devices, uint32_t* leg, double* predicted_us);
int stormck_route_plan_commit(const stormck_dirty_block* blocks, uint64_t n, uint32_t memory, uint32_t host_threads,
                              uint32_t n_devices, uint32_t* leg, double* predicted_us);
/* The split leg alone. base: pinned or registered host memory (pageable is STORMCK_EINVAL:
 * the devices would need host threads to copy it, which hash faster than they copy).
 * devices / n_devices: the devices that take part (NULL / 0: the route devices);
 * host_threads: 0 = the pool. device_blocks: STORMCK_SPLIT_BALANCED to size the devices'
 * chunks from the rates as they run; otherwise exactly the last device_blocks blocks go to
 * the devices and the others to the host threads (tests, A/B). *device_done (optional):
 * blocks the devices hashed. Results and errors as stormck_checksum_host / _verify_host
 * (first_bad is the lowest mismatching index over both sides, n_bad their sum). */
#define STORMCK_SPLIT_BALANCED UINT64_MAX
int stormck_checksum_split(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                           uint64_t* out, const int* devices, int n_devices, uint32_t host_threads,
                           uint64_t device_blocks, uint64_t* device_done);
int stormck_verify_split(const void* base, uint64_t stride, const uint32_t* lens, uint32_t len, uint64_t n,
                         const uint64_t* expected, uint64_t* first_bad, uint64_t* n_bad, const int* devices,
                         int n_devices, uint32_t host_threads, uint64_t device_blocks, uint64_t* device_done);
/* A commit with its leaves (height 0) split: the same rules, order, relocation, stores,
 * outputs and errors as stormck_commit_host, with `arena` registered host memory; the
 * devices hash leaves from the back of the leaf height in place and the host threads store
 * every Pointer (cache/trace.go:274-320); the upper heights (a few pointer blocks) run on
 * the host threads. device_leaves: STORMCK_SPLIT_BALANCED or the exact number of leaves, the
 * last ones of the commit order, the devices hash; *device_done (optional): leaves they
 * hashed. */
int stormck_commit_split(void* arena, stormck_dirty_block* blocks, uint64_t n, uint64_t revision,
                         uint64_t* last_allocated_block, uint64_t* out_checksums, const int* devices, int n_devices,
                         uint32_t host_threads, uint64_t device_leaves, uint64_t* device_done);

/* ---- scrub: verify a whole snapshot from its singularity block ---------------
 * In storm a block's expected checksum lives in its parent (cache/trace.go:10-42,
 * cache/cache.go:157-162), so the integrity of a snapshot is a level-synchronous descent:
 * the mirror image of the commit. The image holds block `a` at store + a * block_size.
 *
 *   singularity (address 0)  72 B hashed with Checksum (bytes 0..7) zeroed; origin of the
 *                            space tree: SpacePointer @32, SpaceBlockType @56
 *   pointer.Block, fanout F  (25*F+7)&~7 B; entry i = Pointers[i] @24*i, type byte @24*F+i:
 *                            0 Free (skipped), 1 a pointer block of the same tree, 2 its leaf
 *   spacelist.Block, S       (72*S+2+7)&~7 B; space k @72*k: KeyStorePointer @16,
 *                            ObjectStorePointer @40, their type bytes @64 / @65, State @66;
 *                            only spaces with State == 1 (Defined) are followed: a key tree
 *                            with objectlist leaves and an object tree with blob leaves
 *   objectlist / blob        objectlist_len / blob_len B, no children
 *
 * A reference is (parent address, slot): the pointer index in a pointer block, 2*k (key
 * tree) or 2*k+1 (object tree) in a spacelist block, (0, 0) for the root. Its level is the
 * referenced block's depth below the root (the root is level 0). Rules, in this order:
 *   TYPE       a type byte above 2, or a State above 2 (reported once, at slot 2*k)
 *   RANGE      the address is 0 or >= n_blocks (tested before any multiplication)
 *   DUPLICATE  the address was referenced before in this scrub: at a shallower level, or at
 *              the same level by a smaller (parent, slot)
 *   MISMATCH   the block's checksum differs from the one its parent holds
 * A reference that breaks a rule is never read; a block that mismatches is counted and
 * never expanded; the walk goes on over everything reachable through verified blocks.
 * The first error is the one at the shallowest level, and within it the smallest (parent,
 * slot), whatever order the blocks were visited in. */
#define STORMCK_HAS_SCRUB 1
typedef struct stormck_scrub_layout {
    uint64_t block_size;        /* 32768 */
    uint64_t n_blocks;          /* addresses 0..n_blocks-1 exist in the image (at most 2^36) */
    uint32_t pointer_fanout;    /* 1200; 10 under -tags test */
    uint32_t spaces_per_block;  /* 400; 10 */
    uint32_t objectlist_len;    /* 31808; 536 */
    uint32_t blob_len;          /* 32768 */
} stormck_scrub_layout;

enum { STORMCK_SCRUB_POINTER, STORMCK_SCRUB_SPACELIST, STORMCK_SCRUB_OBJECTLIST, STORMCK_SCRUB_BLOB };
enum { STORMCK_SCRUB_OK, STORMCK_SCRUB_MISMATCH, STORMCK_SCRUB_RANGE, STORMCK_SCRUB_TYPE, STORMCK_SCRUB_DUPLICATE };

typedef struct stormck_scrub_report {
    uint64_t verified[4];   /* blocks whose checksum matched, per kind above */
    uint64_t bytes_hashed;  /* of every block read, the singularity's 72 included */
    uint64_t n_mismatch;    /* referenced, in range, checksum differs: not expanded */
    uint64_t n_structural;  /* references not followed: RANGE, TYPE, DUPLICATE */
    uint32_t levels;        /* frontier levels hashed */
    uint32_t first_error;   /* STORMCK_SCRUB_*; the fields below describe it */
    uint32_t first_level, first_slot;
    uint64_t first_parent, first_address, first_computed, first_expected; /* the last two: MISMATCH only */
} stormck_scrub_report;

/* Bytes of device workspace a scrub of n_blocks needs: 256 + 57 per block + the visited
 * bitmap (DESIGN.md "Scrub"). Host logic. */
uint64_t stormck_scrub_workspace_bytes(uint64_t n_blocks);
/* Scrub the image at d_store from its singularity: the 72-byte singularity is read back and
 * verified on the host (a failure is MISMATCH at address 0, and nothing else is walked), then
 * the space tree, its spacelist leaves and every Defined space's two trees are walked on the
 * device, one frontier level per step: the level is hashed by the batch dispatch
 * (stormck_checksum_gather_device's), then k_scrub_expand compares, validates and builds the
 * next level. d_store and d_workspace are 8-byte aligned, block_size a multiple of 8.
 * d_reachable (optional): (n_blocks+31)/32 words; bit a is set iff block a was referenced,
 * in range and referenced for the first time (read, whether or not it then matched); bit 0
 * is always set, so popcount = 1 + sum(verified) + n_mismatch (a singularity that fails is
 * bit 0 itself). Synchronous: queues its work on `stream` behind what is already there and
 * returns when the walk has finished. Returns STORMCK_EMISMATCH if n_mismatch +
 * n_structural > 0, with the report filled and the first error's text in
 * stormck_last_error(); STORMCK_EINVAL for null pointers, a zero fanout, lengths above
 * block_size, a small workspace or a stream that is being captured. */
int stormck_scrub_device(const void* d_store, const stormck_scrub_layout* layout, void* d_workspace,
                         uint64_t workspace_bytes, uint32_t* d_reachable, stormck_scrub_report* report, void* stream);
/* One tree from an explicit root of type root_type (Free: nothing to walk). leaf_kind: the
 * kind of its leaves (STORMCK_SCRUB_SPACELIST / _OBJECTLIST / _BLOB; spacelist leaves are
 * expanded); leaf_len overrides the layout's length for that kind (0: the layout's), so shard
 * trees and test trees of any leaf size can be scrubbed. */
int stormck_scrub_tree_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                              uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, void* d_workspace,
                              uint64_t workspace_bytes, uint32_t* d_reachable, stormck_scrub_report* report, void* stream);
/* The same walks over an image in host memory (storm's stores are host memory or files), each
 * level hashed on host_threads library pool threads (0 = the pool). Same rules, report, bitmap
 * and return codes; needs no device and is not routed. */
int stormck_scrub_host(const void* store, const stormck_scrub_layout* layout, uint32_t* reachable,
                       stormck_scrub_report* report, uint32_t host_threads);
int stormck_scrub_tree_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                            uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, uint32_t* reachable,
                            stormck_scrub_report* report, uint32_t host_threads);

/* ---- trace: storm's read path for many tags at once ----------------------------
 * cache.TraceTagForReading (cache/trace.go:10-42) walks from a BlockOrigin down the pointer
 * blocks, taking index = reminder % PointersPerBlock and reminder /= PointersPerBlock per
 * level, and fetchBlock verifies every block on the way against the checksum its parent
 * holds. This is that walk for n tags at once, level by level: one hash batch per tree level
 * instead of one block per key per level. One tree is traced from an explicit root, as
 * stormck_scrub_tree_* walks it: layout, root, root_type, leaf_kind and leaf_len mean what they
 * mean there and take the same argument checks (a leaf is never expanded, whatever its kind).
 *
 * For tag t the walk starts at the root reference (parent 0, slot 0, depth 0, reminder t).
 * A reference is handled by these rules, in this order:
 *   ABSENT    the type byte is Free (storm returns exists == false)
 *   TYPE      the type byte is above 2
 *   RANGE     the address is 0 or >= n_blocks (tested before any multiplication; never read)
 *   DEPTH     the reference is of Pointer type and 64 pointer blocks have already been verified
 *             on this walk (a fanout of at least 2 leaves reminder 0 after 64 digits; storm
 *             itself would spin on a cycle of verified blocks)
 *   MISMATCH  the block, hashed over the pointer-block length or the leaf length, differs
 *             from the checksum the reference holds
 *   FOUND     the block is a verified leaf
 * A verified pointer block at `address` continues the walk: depth += 1, slot = reminder %
 * fanout, reminder /= fanout, and the next reference is entry `slot` of that block (parent =
 * address). MISMATCH, RANGE and TYPE have the scrub's numbers.
 *
 * A block is hashed once per distinct reference (depth, parent, slot), however many tags pass
 * through it; blocks_hashed counts exactly those references. */
#define STORMCK_HAS_TRACE 1
enum {
    STORMCK_TRACE_FOUND = 0,
    STORMCK_TRACE_MISMATCH = 1,
    STORMCK_TRACE_RANGE = 2,
    STORMCK_TRACE_TYPE = 3,
    STORMCK_TRACE_ABSENT = 5,
    STORMCK_TRACE_DEPTH = 6
};
/* A leaf reference ends FOUND without being hashed (after the TYPE and RANGE rules): for
 * callers that read the leaf elsewhere, e.g. from a file with stormck_read_verify_fd against
 * the checksum the parent holds, which d_leaf_checksums returns. */
#define STORMCK_TRACE_LEAVES_UNVERIFIED 1u

typedef struct stormck_trace_result {
    uint64_t address;   /* the block the final reference names (as read, also when RANGE/TYPE); 0 for a Free root */
    uint64_t reminder;  /* the tag reminder where the walk ended (storm's tagReminder for FOUND) */
    uint64_t parent;    /* the block that holds the final reference, 0 = the caller's root */
    uint32_t slot;      /* its slot there: together the BlockOrigin of the leaf or of the Free entry */
    uint16_t depth;     /* pointer blocks verified on the way */
    uint8_t status, reserved;
} stormck_trace_result;

typedef struct stormck_trace_report {
    uint64_t n_status[7];       /* tags per STORMCK_TRACE_* status */
    uint64_t blocks_hashed[2];  /* distinct references hashed: pointer blocks, leaves */
    uint64_t bytes_hashed;
    uint64_t first_bad;         /* the smallest tag index that ended MISMATCH, RANGE, TYPE or DEPTH; n if none */
    uint32_t levels, reserved;  /* tree levels hashed */
} stormck_trace_report;

/* Bytes of device workspace a trace of n_tags needs: 256 + 12 * T + 118 * ((n_tags + 7) & ~7),
 * T = the smallest power of two that is at least 64 and at least 2 * n_tags (the table of
 * distinct references); at most 166 bytes per tag, whatever the image's size (DESIGN.md
 * "Trace"). Host logic. */
uint64_t stormck_trace_workspace_bytes(uint64_t n_tags);
/* Trace the n tags at d_tags through the tree at `root` of the device-resident image d_store.
 * d_results gets one result per tag, in the tags' order. d_leaf_checksums (optional, n u64):
 * per FOUND tag the checksum its parent holds for the leaf, 0 for every other tag.
 * Per level the distinct references are hashed by the batch dispatch
 * (stormck_checksum_gather_device's), then k_trace_step ends or advances every live tag.
 * Synchronous: queues its work on `stream` behind what is already there and returns when the
 * results are in d_results and the report is filled. n == 0 is a no-op with a zero report;
 * at most 2^31 tags per call. d_store, d_tags, d_results, d_leaf_checksums and d_workspace
 * are 8-byte aligned. Returns STORMCK_EMISMATCH when first_bad < n, with the text of tag
 * first_bad's error in stormck_last_error(); ABSENT is not an error. STORMCK_EINVAL for the
 * scrub-tree argument errors, an unknown flag, a small workspace, misaligned pointers or a
 * stream that is being captured. */
int stormck_trace_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                         uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* d_tags, uint64_t n,
                         uint32_t flags, stormck_trace_result* d_results, uint64_t* d_leaf_checksums, void* d_workspace,
                         uint64_t workspace_bytes, stormck_trace_report* report, void* stream);
/* The same trace over an image in host memory with host pointers throughout, each level's
 * distinct blocks hashed on host_threads library pool threads (0 = the pool). Same rules,
 * results, report and return codes; needs no device and no workspace, and is not routed. */
int stormck_trace_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                       uint8_t root_type, uint32_t leaf_kind, uint32_t leaf_len, const uint64_t* tags, uint64_t n,
                       uint32_t flags, stormck_trace_result* results, uint64_t* leaf_checksums,
                       stormck_trace_report* report, uint32_t host_threads);

/* ---- lookup: keystore.GetObjectID for many keys at once ---------------------------
 * keystore.GetObjectID (keystore/keystore.go:18-45) hashes the key to a tag, runs
 * TraceTagForReading down to the objectlist leaf and probes that leaf by open addressing
 * (findChunkPointerForKey and verifyKeyInChunks, keystore.go:112-133,178-208), returning
 * ObjectLinks[index]. This is the three stages for n keys in one call: the key tags
 * (stormck_key_tags_device's launch), the trace above over those tags with objectlist leaves
 * of layout->objectlist_len bytes, and one probe per key.
 *
 * The leaf is objectlist.Block with C = chunks_per_block (blocks/objectlist/block.go:29-40):
 * Blob at 0, KeyTagReminders at 32C, ObjectLinks at 40C, ChunkPointers at 48C,
 * NextChunkPointers at 50C, ChunkPointerStates at 52C, NUsedChunks at 53C, FreeChunkIndex at
 * 53C+2; (53C + 4 + 7) & ~7 bytes, which layout->objectlist_len must equal.
 *
 * The probe, storm's literally: seed = reminder % C; for i = 0..C-1, index = (seed +
 * addressing_offsets[i]) % C and probes = i + 1. A Defined slot (state 1) matches when
 * KeyTagReminders[index] == reminder and the chunk chain at ChunkPointers[index] spells the
 * key: FOUND, object_id = ObjectLinks[index]. An Invalid slot (2) is remembered (the first
 * one). A Free slot (0) ends the probe: ABSENT, index = the remembered Invalid slot or else
 * this one, the slot findChunkPointerForKey hands EnsureObjectID. Any other state byte is
 * skipped. All C slots seen: ABSENT, index = STORMCK_LOOKUP_NO_SLOT, probes = C.
 * The chain: NextChunkPointers[chunk] > C marks the last chunk, which holds that value - C
 * bytes, and the key matches iff exactly that many key bytes remain and are equal; otherwise
 * 32 bytes are compared and the walk moves to the next chunk.
 * The probe never reads outside the leaf and every loop is bounded (C slots; per item 8 chunks
 * of 32 key bytes and the one that ends the chain). Where storm would index or slice out of
 * range (a chunk index >= C, a remaining length above 32, a chunk that is not the last when
 * fewer than 32 key bytes remain) the item does not match, the probe goes on and the key
 * counts in n_malformed.
 *
 * The final status of a key, in this order: STORMCK_LOOKUP_KEY when its length is outside
 * 1..256 (it is hashed and traced like any other, so report.trace counts it, but it is never
 * probed and every other field of its result is 0, index NO_SLOT; its length's bytes must
 * still be readable); the trace's status when that is not FOUND; else the probe's FOUND or
 * ABSENT. With STORMCK_TRACE_LEAVES_UNVERIFIED the leaf is probed without being hashed
 * (storm's warm GetObjectID); the bounds above make that safe on any bytes.
 *
 * The library ships no addressing table: storm's is rand.New(rand.NewSource(0)).Perm(600)
 * from Go's math/rand, and the caller passes it (the Go binding passes
 * objectlist.AddressingOffsets). */
#define STORMCK_HAS_LOOKUP 1
#define STORMCK_LOOKUP_KEY 7            /* key length outside 1..256 (keystore.go:23-28) */
#define STORMCK_LOOKUP_NO_SLOT UINT32_MAX
typedef struct stormck_objectlist_params {
    const uint16_t* addressing_offsets; /* HOST pointer, chunks_per_block entries, a permutation of 0..C-1:
                                           objectlist.AddressingOffsets */
    uint32_t chunks_per_block;          /* 600; 10 under -tags test; 1..4096 */
    uint32_t reserved;
} stormck_objectlist_params;
typedef struct stormck_lookup_result {  /* 32 bytes */
    uint64_t object_id;   /* FOUND: ObjectLinks[index]; otherwise 0 */
    uint64_t address;     /* the trace's final address for this key */
    uint64_t reminder;    /* the trace's reminder */
    uint32_t index;       /* FOUND: the item; probed and ABSENT: the insert slot or NO_SLOT; not probed: NO_SLOT */
    uint16_t probes;      /* slots examined; 0 when the leaf was not probed */
    uint8_t status, reserved;  /* STORMCK_TRACE_* numbers, or STORMCK_LOOKUP_KEY */
} stormck_lookup_result;
typedef struct stormck_lookup_report {
    stormck_trace_report trace;  /* of the trace the call ran, unchanged */
    uint64_t n_status[8];        /* keys per final status */
    uint64_t n_probed, probes;   /* keys whose leaf was probed; sum of their probes */
    uint64_t n_malformed;        /* keys that met at least one malformed chain */
    uint64_t first_bad;          /* smallest key index ending MISMATCH, RANGE, TYPE, DEPTH or KEY; n if none */
} stormck_lookup_report;

/* Bytes of device workspace a lookup of n_keys needs: stormck_trace_workspace_bytes(n_keys)
 * + 40 * ((n_keys + 7) & ~7) (the tags and the trace results, used when the caller passes
 * none) + ((2 * chunks_per_block + 7) & ~7) (the table) + 256 (the counters). Host logic. */
uint64_t stormck_lookup_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block);
/* Look the n keys up in the key tree at `root` of the device-resident image d_store. Key i is
 * addressed exactly as in stormck_key_tags_device: d_keys + (d_offsets ? d_offsets[i] :
 * i * stride), (d_lens ? d_lens[i] : len) bytes, any alignment. d_results gets one result per
 * key, in the keys' order; d_trace_results and d_tags (both optional, n entries) get the
 * trace's results and the tags. Steps on `stream`: the key-tag launch, the trace's engine,
 * k_lookup_probe with one lane per key, one pinned read-back. Synchronous, like the trace;
 * n == 0 is a no-op with a zero report. flags: STORMCK_TRACE_LEAVES_UNVERIFIED.
 * Returns STORMCK_EMISMATCH when first_bad < n, with that key's text in stormck_last_error():
 * the trace's words for a trace status; for KEY storm's own, "key cannot be empty" or "maximum
 * key component length exceeded, maximum: 256, actual: N". STORMCK_EINVAL, before any work,
 * for every argument error of stormck_trace_device, a uniform len outside 1..256 with d_lens
 * null (and n > 0), layout->objectlist_len != (53C + 4 + 7) & ~7, C outside 1..4096, a null table, a
 * table that is not a permutation of 0..C-1, a workspace that is too small, misaligned
 * pointers (8 bytes; d_lens 4). */
int stormck_lookup_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                          uint8_t root_type, const stormck_objectlist_params* params, const void* d_keys,
                          uint64_t stride, const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t len, uint64_t n,
                          uint32_t flags, stormck_lookup_result* d_results, stormck_trace_result* d_trace_results,
                          uint64_t* d_tags, void* d_workspace, uint64_t workspace_bytes, stormck_lookup_report* report,
                          void* stream);
/* The same lookup over an image in host memory with host pointers throughout: stormck_xxh64,
 * the trace's host leg and the same probe function on host_threads library pool threads
 * (0 = the pool). Same rules, results, report and return codes; needs no device and no
 * workspace, and is not routed. */
int stormck_lookup_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                        uint8_t root_type, const stormck_objectlist_params* params, const void* keys, uint64_t stride,
                        const uint64_t* offsets, const uint32_t* lens, uint32_t len, uint64_t n, uint32_t flags,
                        stormck_lookup_result* results, stormck_trace_result* trace_results, uint64_t* tags,
                        stormck_lookup_report* report, uint32_t host_threads);

/* ---- objects: objectstore.GetObject for many object IDs at once --------------------
 * objectstore.GetObject (objectstore/objectstore.go:15-38) runs TraceTagForReading with the
 * object ID as the tag down to a blob leaf and probes that leaf by open addressing (findObject,
 * objectstore.go:92-123), returning the slot's Object when the slot is Defined. This is the two
 * stages, and the copy of the objects into dense rows, for n object IDs in one call: the trace
 * above over the IDs with blob leaves of layout->blob_len bytes, one probe per ID, one row per
 * ID.
 *
 * The leaf is blob.Block (blocks/blob/block.go:25-29): Data[blob_len - 8], then NUsedSlots as
 * u64. findObject views Data as N = objects_per_block values of Go's blob.Object[T]. With
 * S = object_size = unsafe.Sizeof(T), slot k lies at Data + k * stride:
 *   ObjectIDTagReminder u64 at 0, Object at 8 (S bytes), State byte at 8 + S,
 *   stride = (8 + S + 1 + 7) & ~7.
 * Go places each field at the next multiple of its alignment and rounds the struct's size up to
 * its largest alignment: the u64 makes that 8, T at 8 is aligned for every alignment up to 8,
 * S is a multiple of T's alignment so the State byte follows T directly, and 8 + S + 1 rounds
 * up to 8. This holds for every T of alignment at most 8.
 *
 * The probe, storm's literally: start = reminder % N; for j = 0..N-1, k = (start + j) % N and
 * probes = j + 1. A Defined slot (state 1) with ObjectIDTagReminder == reminder: FOUND,
 * index = k. An Invalid slot (2) is remembered (the first one). A Free slot (0) ends the probe:
 * ABSENT, index = the remembered Invalid slot or else this one, the slot findObject hands
 * SetObject. Any other state byte is skipped. All N slots seen: ABSENT, index =
 * STORMCK_LOOKUP_NO_SLOT, probes = N. Every index is below N and N * stride <= blob_len - 8 is
 * checked first, so the probe never leaves the leaf and its loop is bounded.
 *
 * The final status of an ID: the trace's status when that is not FOUND (index NO_SLOT, probes
 * 0); else the probe's FOUND or ABSENT. With STORMCK_TRACE_LEAVES_UNVERIFIED the leaf is
 * probed and read without being hashed (storm's warm GetObject); the bounds above make that
 * safe on any bytes.
 *
 * Row i of the objects array is at objects + i * out_stride. Its first S bytes are the object
 * when ID i is FOUND and zeros otherwise (Go returns the zero T); bytes S..out_stride of a row
 * are never written. objects may be NULL: only the results are written. */
#define STORMCK_HAS_OBJECTS 1
typedef struct stormck_blob_params {
    uint32_t objects_per_block;  /* N, 1..4095 */
    uint32_t object_size;        /* S = unsafe.Sizeof(T), at least 1; N * stride <= layout->blob_len - 8 */
} stormck_blob_params;
typedef struct stormck_object_result {  /* 32 bytes */
    uint64_t object_id;   /* the ID as read */
    uint64_t address;     /* the trace's final address for this ID */
    uint64_t reminder;    /* the trace's reminder */
    uint32_t index;       /* FOUND: the slot; probed and ABSENT: the insert slot or NO_SLOT; not probed: NO_SLOT */
    uint16_t probes;      /* slots examined; 0 when the leaf was not probed */
    uint8_t status, reserved;  /* STORMCK_TRACE_* numbers */
} stormck_object_result;
typedef struct stormck_objects_report {
    stormck_trace_report trace;  /* of the trace the call ran, unchanged */
    uint64_t n_status[8];        /* IDs per final status */
    uint64_t n_probed, probes;   /* IDs whose leaf was probed; sum of their probes */
    uint64_t first_bad;          /* smallest index ending MISMATCH, RANGE, TYPE or DEPTH; n if none */
} stormck_objects_report;

/* Bytes of device workspace a call with n_ids needs: stormck_trace_workspace_bytes(n_ids)
 * + 32 * ((n_ids + 7) & ~7) (the trace results) + 256 (the counters). Host logic. */
uint64_t stormck_objects_workspace_bytes(uint64_t n_ids);
/* Get the objects of n IDs from the object tree at `root` of the device-resident image d_store.
 * ID i is the u64 at d_ids + i * id_stride (id_stride a multiple of 8, at least 8: 32 reads the
 * object_id field of a stormck_lookup_result array in place). d_results gets one result per ID,
 * in the IDs' order, and must not overlap d_ids: with id_stride above 8 its first 8 n bytes hold
 * the gathered IDs while the trace runs (the trace reads dense tags, the workspace formula
 * below has no 8 n bytes that are free during the trace, and a trace that ends every tag at its
 * root writes trace result t as it reads tag t, so the trace-results region cannot lend them);
 * after a call that fails with another code than STORMCK_EMISMATCH d_results is unspecified; d_objects (optional) gets the rows, n * out_stride bytes at any
 * alignment. Steps on `stream`: the trace's engine, k_object_fetch with one lane per ID (the
 * probe, the counters, then the move of the objects: each lane its own, or the
 * whole wave one row at a time, by the object's size: DESIGN.md "Objects"), one pinned
 * read-back. Synchronous, like the trace; n == 0 is a no-op with a zero report. flags:
 * STORMCK_TRACE_LEAVES_UNVERIFIED.
 * Returns STORMCK_EMISMATCH when first_bad < n, with the trace's text for that ID in
 * stormck_last_error(); ABSENT is not an error. STORMCK_EINVAL, before any work, for every
 * argument error of stormck_trace_device, N outside 1..4095, S == 0, N * stride >
 * layout->blob_len - 8, out_stride < S (when d_objects is given), id_stride below 8 or not a
 * multiple of 8, a workspace that is too small, misaligned pointers (d_store, d_ids, d_results,
 * d_workspace: 8 bytes). */
int stormck_objects_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                           uint8_t root_type, const stormck_blob_params* params, const void* d_ids, uint64_t id_stride,
                           uint64_t n, uint32_t flags, stormck_object_result* d_results, void* d_objects,
                           uint64_t out_stride, void* d_workspace, uint64_t workspace_bytes,
                           stormck_objects_report* report, void* stream);
/* The same over an image in host memory with host pointers throughout: the trace's host leg and
 * the same probe function on host_threads library pool threads (0 = the pool). Same rules,
 * results, rows, report and return codes; needs no device and no workspace, and is not routed. */
int stormck_objects_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                         uint8_t root_type, const stormck_blob_params* params, const void* ids, uint64_t id_stride,
                         uint64_t n, uint32_t flags, stormck_object_result* results, void* objects, uint64_t out_stride,
                         stormck_objects_report* report, uint32_t host_threads);

/* ---- spaces: spacestore.GetSpace for space IDs --------------------------------------
 * spacestore.GetSpace (spacestore/spacestore.go:14-42) runs TraceTagForReading with the space ID
 * as the tag down to a spacelist leaf and probes that leaf by open addressing (findSpace,
 * spacestore.go:92-121); a Defined space holds the two tree roots of the space. This is both
 * stages for n space IDs in one call: the trace above over the IDs (n dense u64) with spacelist
 * leaves of (72 * spaces_per_block + 2 + 7) & ~7 bytes, and one probe per ID.
 *
 * A space is 72 bytes (blocks/spacelist/block.go:21-31): SpaceIDTagReminder at 0, NextObjectID
 * at 8, KeyStorePointer at 16, ObjectStorePointer at 40, KeyStoreBlockType at 64,
 * ObjectStoreBlockType at 65, State at 66.
 *
 * The probe, storm's literally, with S = layout->spaces_per_block: seed = reminder % S; for
 * i = 0..S-1, index = (seed + addressing_offsets[i]) % S and probes = i + 1. A Defined space
 * (state 1) with SpaceIDTagReminder == reminder: FOUND. An Invalid space (2) is remembered (the
 * first one). A Free space (0) ends the probe: ABSENT, index = the remembered Invalid slot or
 * else this one, the slot findSpace hands EnsureSpace. Any other state byte is skipped. All S
 * slots seen: ABSENT, index = STORMCK_LOOKUP_NO_SLOT, probes = S. Every index is below S, so the
 * probe never leaves the leaf and its loop is bounded: STORMCK_TRACE_LEAVES_UNVERIFIED is safe
 * on any bytes. ABSENT is storm's "space does not exist".
 *
 * addressing_offsets is the caller's spacelist.AddressingOffsets: a HOST pointer to
 * spaces_per_block entries, checked to be a permutation of 0..S-1. The library ships no table,
 * for the reason the lookup gives. S is at most 32768 here (storm computes the index in uint16). */
#define STORMCK_HAS_SPACES 1
typedef struct stormck_space_result {  /* 88 bytes */
    stormck_pointer key_root;     /* FOUND: KeyStorePointer; otherwise zeros */
    stormck_pointer object_root;  /* FOUND: ObjectStorePointer; otherwise zeros */
    uint64_t next_object_id;      /* FOUND: NextObjectID; otherwise 0 */
    uint64_t address;             /* the trace's final address for this ID */
    uint64_t reminder;            /* the trace's reminder */
    uint32_t index;               /* FOUND: the slot; probed and ABSENT: the insert slot or NO_SLOT; not probed: NO_SLOT */
    uint16_t probes;              /* slots examined; 0 when the leaf was not probed */
    uint8_t key_type, object_type;  /* FOUND: the two block types; otherwise 0 */
    uint8_t status;               /* STORMCK_TRACE_* numbers */
    uint8_t reserved[7];
} stormck_space_result;
typedef struct stormck_spaces_report {
    stormck_trace_report trace;  /* of the trace the call ran, unchanged */
    uint64_t n_status[8];        /* IDs per final status */
    uint64_t n_probed, probes;   /* IDs whose leaf was probed; sum of their probes */
    uint64_t first_bad;          /* smallest index ending MISMATCH, RANGE, TYPE or DEPTH; n if none */
} stormck_spaces_report;

/* Bytes of device workspace a call with n_ids needs: stormck_trace_workspace_bytes(n_ids)
 * + 32 * ((n_ids + 7) & ~7) (the trace results) + ((2 * spaces_per_block + 7) & ~7) (the
 * table) + 256 (the counters). Host logic. */
uint64_t stormck_spaces_workspace_bytes(uint64_t n_ids, uint32_t spaces_per_block);
/* Get the spaces of the n IDs at d_ids from the space tree at `root` of the device-resident
 * image d_store. Steps on `stream`: the table's upload, the trace's engine, k_space_probe with
 * one lane per ID, one pinned read-back. Synchronous, like the trace; n == 0 is a no-op with a
 * zero report. flags: STORMCK_TRACE_LEAVES_UNVERIFIED. Returns STORMCK_EMISMATCH when
 * first_bad < n, with the trace's text for that ID in stormck_last_error(). STORMCK_EINVAL,
 * before any work, for every argument error of stormck_trace_device, spaces_per_block above
 * 32768, a null table, a table that is not a permutation, a workspace that is too small,
 * misaligned pointers (8 bytes). */
int stormck_spaces_device(const void* d_store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                          uint8_t root_type, const uint16_t* addressing_offsets, const uint64_t* d_ids, uint64_t n,
                          uint32_t flags, stormck_space_result* d_results, void* d_workspace, uint64_t workspace_bytes,
                          stormck_spaces_report* report, void* stream);
/* The same over an image in host memory with host pointers throughout. Same rules, results,
 * report and return codes; needs no device and no workspace, and is not routed. */
int stormck_spaces_host(const void* store, const stormck_scrub_layout* layout, const stormck_pointer* root,
                        uint8_t root_type, const uint16_t* addressing_offsets, const uint64_t* ids, uint64_t n,
                        uint32_t flags, stormck_space_result* results, stormck_spaces_report* report,
                        uint32_t host_threads);

/* ---- get: storm.Get for many keys of one space ---------------------------------------
 * storm.Get (storm.go:32-58) is spacestore.GetSpace, keystore.GetObjectID and
 * objectstore.GetObject, one after the other. This is the three stages for n keys of one space
 * in one call, from the store's singularity block:
 *   1. the singularity (block 0, 72 bytes) is read and verified on the host as the scrub
 *      verifies it; a failure is MISMATCH at stage 0 for every key;
 *   2. "spaces" above with n = 1: space_id from the singularity's space origin;
 *   3. "lookup" above over the keys from the space's key root;
 *   4. the keys whose lookup ended FOUND are compacted, in their order, into a dense ID array;
 *   5. "objects" above over those IDs from the space's object root;
 *   6. results and object rows go back to key order; rows of keys without an object are zeros
 *      over object_size bytes, bytes past object_size of a row are never written, d_objects may
 *      be NULL.
 * The status of a key, with the stage where its walk ended: the space's status when that is not
 * FOUND (stage 0; all keys share it; ABSENT there is storm's "space does not exist"); else the
 * lookup's status when that is not FOUND (stage 1); else the object stage's status (stage 2: a
 * key that is present whose object slot is not Defined ends ABSENT there).
 * first_bad is the smallest key index ending MISMATCH, RANGE, TYPE, DEPTH or KEY; the call then
 * returns STORMCK_EMISMATCH with that key's text in stormck_last_error(): the scrub's words for
 * the singularity, the spaces call's, the lookup's, or the object trace's (the compaction keeps
 * the keys' order, so the object trace's own first bad ID is that key).
 * STORMCK_TRACE_LEAVES_UNVERIFIED applies to objectlist and blob leaves alike (storm's warm Get);
 * the spacelist leaf is always verified. */
#define STORMCK_HAS_GET 1
typedef struct stormck_get_params {
    const uint16_t* space_offsets;   /* HOST pointer: spacelist.AddressingOffsets, layout->spaces_per_block entries */
    stormck_objectlist_params keys;  /* the lookup's */
    stormck_blob_params objects;     /* the objects call's */
} stormck_get_params;
typedef struct stormck_get_result {  /* 32 bytes */
    uint64_t object_id;       /* the lookup's object ID; 0 when the key has none */
    uint64_t key_address;     /* stage 1 and 2: the lookup's final address for the key; stage 0: 0 */
    uint64_t object_address;  /* stage 2: the object trace's final address; otherwise 0 */
    uint32_t index;           /* stage 2: the object stage's index; stage 1: the lookup's; stage 0: NO_SLOT */
    uint8_t stage;            /* 0 space, 1 key, 2 object: where the walk ended */
    uint8_t status;           /* STORMCK_TRACE_* numbers, or STORMCK_LOOKUP_KEY */
    uint16_t reserved;
} stormck_get_result;
typedef struct stormck_get_report {
    stormck_space_result space;    /* the one space's result (zeros when the singularity failed) */
    stormck_lookup_report lookup;  /* of the lookup the call ran, unchanged (zeros, first_bad n, when it did not run) */
    uint64_t n_selected;           /* keys whose lookup ended FOUND: the object stage's IDs */
    uint64_t n_status[8];          /* the object stage: IDs per status */
    uint64_t blocks_hashed[2];     /* the object stage's trace: pointer blocks, leaves */
    uint64_t bytes_hashed;         /* ... its bytes */
    uint64_t probes;               /* ... sum of its probes */
    uint32_t levels, reserved;     /* ... its tree levels */
    uint64_t n_found;              /* keys that ended FOUND at stage 2 */
    uint64_t first_bad;            /* in key indices; n if none */
} stormck_get_report;

/* Bytes of device workspace a call with n_keys needs: stormck_lookup_workspace_bytes(n_keys,
 * chunks_per_block) (the lookup's, which the spaces and the objects stage reuse)
 * + stormck_spaces_workspace_bytes(1, 32768) when that is larger + 80 * ((n_keys + 7) & ~7) (the
 * lookup's results, the dense IDs, the object stage's results, each key's place among them and
 * each ID's key) + 8 * (n_keys / 256 + 2) (the compaction's counts) + 128 (the space). Host logic. */
uint64_t stormck_get_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block);
/* Get the objects of n keys (addressed as in stormck_lookup_device) of space space_id in the
 * device-resident store d_store. d_results gets one result per key, d_objects (optional) one row
 * per key, out_stride apart. Synchronous; n == 0 is a no-op with a zero report. STORMCK_EINVAL,
 * before any work, for every argument error of the three calls it contains, a workspace that is
 * too small, misaligned pointers. */
int stormck_get_device(const void* d_store, const stormck_scrub_layout* layout, uint64_t space_id,
                       const stormck_get_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                       const uint32_t* d_lens, uint32_t len, uint64_t n, uint32_t flags, stormck_get_result* d_results,
                       void* d_objects, uint64_t out_stride, void* d_workspace, uint64_t workspace_bytes,
                       stormck_get_report* report, void* stream);
/* The same over a store in host memory with host pointers throughout, through the three host
 * legs. Same rules, results, rows, report and return codes; needs no device and no workspace. */
int stormck_get_host(const void* store, const stormck_scrub_layout* layout, uint64_t space_id,
                     const stormck_get_params* params, const void* keys, uint64_t stride, const uint64_t* offsets,
                     const uint32_t* lens, uint32_t len, uint64_t n, uint32_t flags, stormck_get_result* results,
                     void* objects, uint64_t out_stride, stormck_get_report* report, uint32_t host_threads);

/* ---- update: storm.Set for keys that already have an object, as a new revision ----------
 * storm.Set (storm.go:61-79) is EnsureSpace, EnsureObjectID and SetObject, then Cache.Commit.
 * On a key that already has an object, EnsureSpace and EnsureObjectID find what GetSpace and
 * GetObjectID find, and SetObject (objectstore/objectstore.go:41-90) sees a Defined slot: it
 * stores the object and commits the trace; NUsedSlots, the state byte and the reminder stay,
 * and no block is allocated or split. Cache.Commit then rehashes the touched blob leaves, their
 * ancestors in the object tree, the spacelist leaf that holds the space's ObjectStorePointer, its
 * ancestors and the singularity, and moves each of them to a fresh address
 * (cache/cache.go:113-118). This is that case for n keys of one space in one call, in place in
 * the image; everything else of Set (inserts, slots that are not Defined, splits, EnsureSpace)
 * stays storm's. Row i of the objects array is at + i * in_stride, at any alignment; its first
 * S = params->objects.object_size bytes are the new object of key i. flags must be 0: every leaf
 * is verified, because the call re-signs the leaves it writes and must not launder damage.
 *
 * A. Locate (nothing is written). The get above runs over the keys with no rows. results[i]
 *    holds the get's values on the old store. If the get ends STORMCK_EMISMATCH the call
 *    returns that code and text, every action is NONE and the store is byte for byte as it was.
 * B. Select. A key is applicable when it ended FOUND at stage 2. Every other key (an absent
 *    space, an absent key, a key whose object slot is not Defined: storm would insert there)
 *    has action NONE; the caller sends those to storm's own Set. Among the applicable keys that
 *    name one slot (object_address, index) the one with the largest i is WRITTEN, the others
 *    are SUPERSEDED: storm's serial loop, where the last Set wins. With no WRITTEN key the call
 *    returns STORMCK_OK with the store untouched, Revision and LastAllocatedBlock included.
 *    Deviation: storm's Commit would still bump the revision; a batch that changes nothing
 *    makes no revision here.
 * C. Dirty forest. The dirty blocks are the distinct blob leaves of WRITTEN keys, every
 *    pointer block on those object IDs' walks from the space's object root, the spacelist leaf
 *    that holds the space's record, and every pointer block on the space ID's walk from the
 *    singularity's space origin. The height of a dirty block is 0 without a dirty child, else 1
 *    + the largest height among its dirty children (the spacelist leaf's dirty child is the
 *    object tree's root block, which may itself be a leaf). Order: ascending height, within a
 *    height ascending old address. With L = the singularity's LastAllocatedBlock and D dirty
 *    blocks, the k-th block in that order (k from 0) moves to address L + 1 + k. Deviation:
 *    every dirty block moves. storm moves a block only when BirthRevision <= Revision, which
 *    holds for every block of a store that storm's commit wrote; the call does not look at the
 *    field. If L + D >= layout->n_blocks (the image's capacity) or L >= layout->n_blocks the
 *    call returns STORMCK_ENOSPC with the store untouched.
 * D. Write. Steps 1 to 3 go only to addresses above L; the singularity is last.
 *    1. Each dirty block's whole block_size bytes are copied from its old address to its new.
 *    2. The S bytes of each WRITTEN key's row are stored at the object of slot `index` in the
 *       new leaf. Nothing else of the slot changes, and NUsedSlots does not.
 *    3. The commit above runs over the new copies, children first by height: each dirty block
 *       is hashed at its new address over its kind's length, and Pointer{checksum, new address,
 *       Revision + 1} and the block's unchanged type byte are stored into the origin in the
 *       parent's new copy: entry `slot` of a pointer block; ObjectStorePointer @72k+40 and its
 *       type @72k+65 of the space's record; SpacePointer @32 and its type @56 of the
 *       singularity's host copy.
 *    4. The singularity: Revision + 1, LastAllocatedBlock = L + D, Checksum over the 72 bytes
 *       with the field zeroed, written as 72 bytes to block 0 as the call's last store. The rest
 *       of block 0 is not touched.
 * Three consequences. The old snapshot survives: every byte of blocks 1..L is unchanged, and
 * putting the old 72 bytes back into block 0 gives back the old store. Failure is all or
 * nothing: a HIP error before step 4 leaves the old revision valid. Writes stay in bounds: no
 * byte at or beyond n_blocks * block_size is written, and none in blocks (L + D, n_blocks).
 * Everything storm shares between revisions stays shared: the key tree, untouched object
 * leaves, other spaces. The old blocks are not reclaimed. */
#define STORMCK_HAS_UPDATE 1
#define STORMCK_ENOSPC (-6)  /* update: the image has no room for the dirty blocks */
enum { STORMCK_UPDATE_NONE = 0, STORMCK_UPDATE_WRITTEN = 1, STORMCK_UPDATE_SUPERSEDED = 2 };
typedef struct stormck_update_result {  /* 32 bytes: stormck_get_result with its reserved field split */
    uint64_t object_id;
    uint64_t key_address;
    uint64_t object_address;  /* on the old store */
    uint32_t index;
    uint8_t stage;
    uint8_t status;
    uint8_t action;           /* STORMCK_UPDATE_* */
    uint8_t reserved;
} stormck_update_result;
typedef struct stormck_update_report {
    stormck_get_report get;          /* of the get the call ran, unchanged */
    uint64_t n_written, n_superseded;
    uint64_t n_dirty[4];             /* dirty blocks per STORMCK_SCRUB_* kind (objectlist: always 0) */
    uint64_t bytes_copied;           /* D * block_size */
    uint64_t bytes_hashed;           /* of the dirty blocks at their kinds' lengths, and the singularity's 72 */
    uint64_t revision;               /* the singularity's after the call, when the get returned STORMCK_OK; otherwise 0 */
    uint64_t last_allocated;         /* likewise */
    uint64_t first_new;              /* L + 1, or 0 when nothing moved */
    uint32_t heights, reserved;      /* distinct heights of the dirty forest */
} stormck_update_report;

/* Bytes of device workspace a call with n_keys needs: stormck_get_workspace_bytes(n_keys,
 * chunks_per_block) rounded up to 8 + 12 * T (the table of distinct slots and of distinct
 * blocks, T = the smallest power of two that is at least 64 and at least 2 * n_keys) + 24 *
 * (((n_keys + 7) & ~7) + 72) (the dirty blocks of one tree level, and the space's path) + 64
 * (the counters): O(n_keys), whatever the image's size. Host logic. */
uint64_t stormck_update_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block);
/* Update the objects of n keys (addressed as in stormck_lookup_device) of space space_id in the
 * device-resident store d_store, which is written in place. Steps on `stream`: the get; the
 * winner of every slot (k_update_claim, k_update_actions); the dirty blocks, one tree level per
 * launch (k_update_walk), read back as one small record per dirty block; the plan on the host;
 * k_update_copy, k_object_store (each lane its own row, or the whole wave one row at a time, by
 * the object's size as in "objects"); the device commit; the singularity's 72 bytes.
 * Synchronous; n == 0 is a no-op with a zero report. A block deeper than 64 pointer blocks
 * ends the get DEPTH, so the walks are bounded. STORMCK_EINVAL, before any work, for every
 * argument error of the get, flags != 0, in_stride < S, a null d_objects with n > 0, a
 * workspace that is too small, misaligned pointers (8 bytes: d_store, d_results, d_offsets,
 * d_workspace; 4: d_lens), a stream that is being captured. */
int stormck_update_device(void* d_store, const stormck_scrub_layout* layout, uint64_t space_id,
                          const stormck_get_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                          const uint32_t* d_lens, uint32_t len, uint64_t n, const void* d_objects, uint64_t in_stride,
                          uint32_t flags, stormck_update_result* d_results, void* d_workspace, uint64_t workspace_bytes,
                          stormck_update_report* report, void* stream);
/* The same over a store in host memory with host pointers throughout: the get's host leg, the
 * same plan and the commit's host leg on host_threads library pool threads (0 = the pool). Same
 * rules, results, image bytes, report and return codes; needs no device and no workspace. */
int stormck_update_host(void* store, const stormck_scrub_layout* layout, uint64_t space_id,
                        const stormck_get_params* params, const void* keys, uint64_t stride, const uint64_t* offsets,
                        const uint32_t* lens, uint32_t len, uint64_t n, const void* objects, uint64_t in_stride,
                        uint32_t flags, stormck_update_result* results, stormck_update_report* report,
                        uint32_t host_threads);

/* ---- insert: storm.Set for new keys whose leaves have room, as a new revision ------------
 * On a key that is not in the store, storm.Set runs EnsureObjectID (keystore/keystore.go:48-110),
 * which puts the key into its objectlist leaf under the space's NextObjectID, and SetObject
 * (objectstore/objectstore.go:41-90), which puts the object into a slot of the ID's blob leaf.
 * This is that case for n keys of one existing space in one call, in place in the image, for
 * every key that storm would insert without a split and without allocating a leaf. The new
 * store is what storm's serial loop over the accepted keys, in batch order, would leave, under
 * the two deviations of "update" (a batch that changes nothing makes no revision; every dirty
 * block moves). Every other key is NONE with a reason: the caller sends it to the update call
 * (EXISTS) or to storm's own Set. Arguments as in "update"; flags must be 0.
 * chunks_per_block is at most STORMCK_INSERT_MAX_CHUNKS (the device's leaf worker holds a leaf
 * image and its ordering buffer in LDS), else STORMCK_EINVAL. n == 0 is a no-op with a zero report.
 *
 * A. Locate (nothing is written). The singularity's check as in "get", "spaces" with n = 1,
 *    "lookup" over the keys from the space's key root with leaves verified. When a stage returns
 *    STORMCK_EMISMATCH the call returns that code and text, every action is NONE with reason 0
 *    and the store is byte for byte as it was. A space that is not FOUND: every key is NONE /
 *    SPACE, STORMCK_OK, store untouched. Else a key whose lookup ended FOUND is NONE / EXISTS; one
 *    whose trace ended at a Free reference (probes == 0, ABSENT) is NONE / NO_LEAF; one that was
 *    probed and is ABSENT is a candidate.
 * B. Key stage. Each objectlist leaf's candidates are taken in ascending key index, each judged
 *    against the leaf as the earlier ones left it (keystore.go:72-109, literally):
 *    1. findChunkPointerForKey with the key. A Defined match is a key an earlier candidate of the
 *       batch put there: REPEATED, with object_id and key_index of that item.
 *    2. Else NUsedChunks >= C * 3 / 4 (SplitTrigger): NONE / KEY_SPLIT.
 *    3. Else no slot was handed out: NONE / NO_SLOT.
 *    4. Else NUsedChunks + ceil(len / 32) > C: NONE / KEY_FULL.
 *    5. Else setKeyInChunks byte for byte: initFreeChunkList when NUsedChunks == 0; state
 *       Defined, ChunkPointers[index] = FreeChunkIndex, KeyTagReminders[index] = the reminder; the
 *       chunks taken off the free list, each receiving only the key's bytes; the last next
 *       pointer = C + nCopied; ObjectLinks[index] = the key's new ID: INSERTED. Before anything
 *       changes the ceil(len / 32) steps of the free list are walked; a FreeChunkIndex or next
 *       pointer >= C on the way (storm would index out of range) makes the key NONE / MALFORMED
 *       with the leaf as it was before the key.
 *    A leaf with more than STORMCK_INSERT_MAX_PER_LEAF candidates: all of them NONE / CROWDED. A
 *    later, shorter key may be accepted after a KEY_FULL one.
 * C. IDs. The INSERTED keys ranked in key order: rank r gets NextObjectID + r (keystore.go:104-105).
 * D. Object stage (still nothing written). "objects" over the new IDs from the space's object
 *    root, leaves verified; a MISMATCH, RANGE, TYPE or DEPTH there ends the call
 *    STORMCK_EMISMATCH with the trace's text, every action NONE with reason 0, store untouched.
 *    Each blob leaf's IDs are taken in ascending rank against the leaf's slots as the earlier
 *    ones left them (objectstore.go:59-85, literally): findObject; a slot that is nil or not
 *    Defined while NUsedSlots >= N * 3 / 4 fails the rank (storm splits); a nil slot fails it
 *    (storm errors); a Defined slot with the ID's reminder (NextObjectID lags) is overwritten
 *    without counting. A trace that ends at a Free reference fails (storm allocates). A leaf with
 *    more than STORMCK_INSERT_MAX_PER_LEAF IDs fails at its smallest rank. cut = the smallest
 *    failing rank, or the number of INSERTED keys.
 * E. Cut. limit = the key index of the INSERTED key of rank cut (n if none). Every key i >= limit
 *    becomes NONE / CUT with the fields the locate left; the verdicts below limit stand. With no
 *    INSERTED key left: STORMCK_OK, store untouched, Revision included.
 * F. Rows. The slot of an INSERTED key below limit receives the row of that key's last
 *    occurrence below limit (itself or a REPEATED one); that occurrence has wrote = 1 once the
 *    call has written (after STORMCK_ENOSPC no slot received anything and every wrote is 0).
 * G. Dirty forest and plan. Dirty: the objectlist leaves with an INSERTED key and the key
 *    tree's pointer blocks on those keys' walks; the blob leaves of the placed IDs and the object
 *    tree's pointer blocks on their walks; the spacelist leaf and the space ID's path. Heights,
 *    order, new addresses L + 1 + k and STORMCK_ENOSPC as rule C of "update". The spacelist leaf
 *    has up to two dirty children: KeyStorePointer @72k+16 with its type @72k+64,
 *    ObjectStorePointer @72k+40 with its type @72k+65.
 * H. Write, everything above L, the singularity last. A key leaf's new copy is the old leaf with
 *    its inserts; every other dirty block is copied. Blob slots: Object = the row; if the slot
 *    was not Defined, NUsedSlots++, the reminder, state Defined. NextObjectID = old + cut @72k+8
 *    in the spacelist leaf's new copy. Then the commit over the copies and the singularity's 72
 *    bytes. The three consequences of "update" hold unchanged.
 *
 * The result of a key: object_id is the key's ID after the call for INSERTED / REPEATED, the ID
 * it has for EXISTS, else 0. key_address: the lookup's final address. key_index: the item for
 * INSERTED / REPEATED / EXISTS, else the slot the lookup found free (or NO_SLOT). object_address
 * (on the old store) and object_index: the blob leaf and slot of an INSERTED key, else 0 and
 * NO_SLOT. stage / status: 0 and the space's status when the space is not FOUND; 2 and the object
 * stage's (ABSENT, or FOUND for a lagging NextObjectID) for an INSERTED key; else 1 and the
 * lookup's. */
#define STORMCK_HAS_INSERT 1
#define STORMCK_INSERT_MAX_CHUNKS 1024
#define STORMCK_INSERT_MAX_PER_LEAF 2048
enum { STORMCK_INSERT_NONE = 0, STORMCK_INSERT_INSERTED = 1, STORMCK_INSERT_REPEATED = 2 };
enum {
    STORMCK_INSERT_R_NONE = 0,  /* INSERTED, REPEATED, or a call that returned STORMCK_EMISMATCH */
    STORMCK_INSERT_R_SPACE = 1, STORMCK_INSERT_R_EXISTS = 2, STORMCK_INSERT_R_NO_LEAF = 3, STORMCK_INSERT_R_KEY_SPLIT = 4,
    STORMCK_INSERT_R_NO_SLOT = 5, STORMCK_INSERT_R_KEY_FULL = 6, STORMCK_INSERT_R_MALFORMED = 7,
    STORMCK_INSERT_R_CROWDED = 8, STORMCK_INSERT_R_CUT = 9, STORMCK_INSERT_REASONS = 10
};
typedef struct stormck_insert_result {  /* 40 bytes */
    uint64_t object_id;
    uint64_t key_address;
    uint64_t object_address;  /* on the old store */
    uint32_t key_index;
    uint32_t object_index;
    uint8_t stage, status;
    uint8_t action;           /* STORMCK_INSERT_NONE / INSERTED / REPEATED */
    uint8_t reason;           /* STORMCK_INSERT_R_* */
    uint8_t wrote;            /* this key's row is the one its slot received */
    uint8_t reserved[3];
} stormck_insert_result;
typedef struct stormck_insert_report {
    stormck_space_result space;    /* the one space's result (zeros when the singularity failed) */
    stormck_lookup_report lookup;  /* of the lookup the call ran, unchanged (zeros, first_bad n, when it did not run) */
    uint64_t n_inserted, n_repeated;
    uint64_t n_none[STORMCK_INSERT_REASONS];  /* NONE keys per reason */
    uint64_t first_id;               /* NextObjectID before the call; 0 when the space is not FOUND */
    uint64_t next_object_id;         /* ... after it: first_id + cut when something was written, else first_id */
    uint64_t cut, limit;             /* rule E; 0 and n when the key stage did not run */
    uint64_t n_dirty[4];             /* dirty blocks per STORMCK_SCRUB_* kind */
    uint64_t bytes_copied;           /* D * block_size */
    uint64_t bytes_hashed;           /* of the dirty blocks at their kinds' lengths, and the singularity's 72 */
    uint64_t revision;               /* the singularity's after the call, when the locate returned STORMCK_OK; otherwise 0 */
    uint64_t last_allocated;         /* likewise */
    uint64_t first_new;              /* L + 1, or 0 when nothing moved */
    uint32_t heights, reserved;      /* distinct heights of the dirty forest */
} stormck_insert_report;

/* Bytes of device workspace a call with n_keys needs, with m = (n_keys + 7) & ~7 and T = the
 * smallest power of two that is at least 64 and at least 2 * n_keys:
 *   max(stormck_lookup_workspace_bytes(n_keys, C), stormck_spaces_workspace_bytes(1, 32768),
 *       stormck_objects_workspace_bytes(n_keys)) rounded up to 8: the part the three engines use in turn
 * + 32 m (the lookup's results) + 8 m (the keys' tags) + 8 m (the new IDs) + 32 m (the object
 *   stage's results) + 4 m (each key's rank) + 4 m (each rank's key) + 4 m (each key's last occurrence)
 * + 8 m (each item's leaf, for the grouping) + 2 * 4 m (the segments of the key leaves and of the
 *   blob leaves) + 3 * 8 (m + 8) (the addresses of the key leaves and of the blob leaves, and the
 *   key leaves' new addresses) + 3 * 4 (m + 8) (the two groupings' counts, then starts, and the
 *   fill's cursors)
 * + 8 (n_keys / 256 + 2) (the compaction's counts) + 12 T (the table of distinct leaves and
 *   blocks) + 24 (m + 72) (the dirty blocks of one tree level, and the space's path)
 * + ((2 C + 7) & ~7) (the addressing table) + 128 (the space) + 64 + 128 (the counters):
 * O(n_keys), whatever the image's size. Host logic. */
uint64_t stormck_insert_workspace_bytes(uint64_t n_keys, uint32_t chunks_per_block);
/* Insert the n keys (addressed as in stormck_lookup_device) with their rows (as in "update")
 * into space space_id of the device-resident store d_store, which is written in place. Steps on
 * `stream`: the three engines; the grouping of the candidates by leaf (a table, a scan, a fill);
 * k_insert_keys with one workgroup per key leaf on an LDS image of the leaf; the ranks; the
 * objects call over the new IDs; the grouping by blob leaf and k_insert_slots with one wave per
 * leaf; the dirty walks, one tree level per launch; the plan on the host; k_update_copy,
 * k_insert_keys and k_insert_slots again, now writing the new copies; the device commit; the
 * singularity's 72 bytes. Synchronous. STORMCK_EINVAL, before any work, as "update", and for
 * chunks_per_block above STORMCK_INSERT_MAX_CHUNKS. */
int stormck_insert_device(void* d_store, const stormck_scrub_layout* layout, uint64_t space_id,
                          const stormck_get_params* params, const void* d_keys, uint64_t stride, const uint64_t* d_offsets,
                          const uint32_t* d_lens, uint32_t len, uint64_t n, const void* d_objects, uint64_t in_stride,
                          uint32_t flags, stormck_insert_result* d_results, void* d_workspace, uint64_t workspace_bytes,
                          stormck_insert_report* report, void* stream);
/* The same over a store in host memory with host pointers throughout: plain loops over the same
 * rule functions; the library's pool works only inside the lookup, the trace and the commit.
 * Same rules, results, image bytes, report and return codes; needs no device and no workspace. */
int stormck_insert_host(void* store, const stormck_scrub_layout* layout, uint64_t space_id,
                        const stormck_get_params* params, const void* keys, uint64_t stride, const uint64_t* offsets,
                        const uint32_t* lens, uint32_t len, uint64_t n, const void* objects, uint64_t in_stride,
                        uint32_t flags, stormck_insert_result* results, stormck_insert_report* report,
                        uint32_t host_threads);

/* ---- synthetic data (benchmarks / tests) -----------------------------------
 * Word w of block i = splitmix64(seed ^ (((first + i) << 20) + w)), w < stride/8,
 * little-endian. stride % 16 == 0, d_dst 16-byte aligned. */
int stormck_fill_synthetic_device(void* d_dst, uint64_t stride, uint64_t n, uint64_t first, uint64_t seed,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* STORMCK_H */
