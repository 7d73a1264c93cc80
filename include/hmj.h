/*
 * hmj.h -- C ABI of libhmj_hip.so: the MI355X (gfx950) radix-partitioned hash-join executor.
 *
 * This is the drop-in boundary for ONE path of dryman/HashMergeJoin: radix partition ->
 * bucket-local build -> probe, behind the reference's join operator.  Every entry point cites
 * the reference interface it replaces (file:line in the reference tree).  Plain pointers and
 * sizes only; no C++/STL/torch types cross this line; nothing throws.
 *
 * Relation layout (reference: hashjoin.h:29-31 KeyValVec, strgen.h:24-25):
 *   n x { uint64_t key; uint64_t val; }  ==  std::pair<uint64_t,uint64_t>[n], contiguous AoS.
 * Key hash: std::hash<uint64_t>, the identity (radix_hash.h:353) -- partitions are
 * taken from the most significant bits of the key, as the reference does (radix_hash.h:369).
 * R is the build side, S the probe side; a result row is (key, rval, sval) exactly as
 * HashMergeJoin::iterator::operator* yields it (hashjoin.h:168-173).
 *
 * Semantics: relational equi-join.  For relations whose keys are unique within each relation
 * (the reference generator's invariant, strgen_test.cc:24-33) the result equals what iterating
 * the reference's HashMergeJoin yields, and with HMJ_ORDERED the order equals its iteration order
 * (ascending key).  With duplicate keys: cross product per key (or HMJ_FIRST_WINS); the reference
 * iterator's "staircase"/tail-cut artefact is not reproduced.
 *
 * Threading: an hmj_ctx is not thread-safe; use one per calling thread / per GPU.
 */
#ifndef HMJ_H
#define HMJ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hmj_ctx hmj_ctx;

/* status codes: 0 ok, negative = error (the reference has none: assert/UB, strgen.cc:60) */
#define HMJ_OK 0
#define HMJ_E_ARG (-1)         /* bad argument / size beyond 2^32-1 tuples per call */
#define HMJ_E_NODEV (-2)       /* no usable HIP device */
#define HMJ_E_OOM (-3)         /* device or host allocation failed */
#define HMJ_E_HIP (-4)         /* HIP runtime error, see hmj_last_error() */
#define HMJ_E_UNSUPPORTED (-5) /* the flags cannot be honoured for this input (e.g. HMJ_ORDERED with a */
                               /* single partition's result beyond 2^31-1 rows)                      */

#define HMJ_E_RCCL (-6)        /* RCCL (or the host's transport callbacks) failed, or librccl is absent  */
#define HMJ_E_PEER (-7)        /* a collective call failed on ANOTHER rank; every rank returns together   */
#define HMJ_E_TIMEOUT (-8)     /* a step of the exchange made no progress within hmj_comm_set_timeout_ms: a peer */
                               /* never took part (or died).  The communicator is unusable: hmj_comm_destroy it   */

/* flags for hmj_join_* */
#define HMJ_MATERIALIZE 0x01u /* produce the (key, rval, sval) columns; else count/sums only --   */
                              /* the reduction hashjoin_bench.cc:131-133 performs.  Row order is  */
                              /* unspecified without HMJ_ORDERED (a join may come back ordered)   */
#define HMJ_ORDERED 0x02u     /* rows sorted by (key, rval, sval): HashMergeJoin iteration order  */
                              /* (hashjoin.h:104-154); implies HMJ_MATERIALIZE                    */
#define HMJ_FIRST_WINS 0x04u  /* each probe row pairs with the FIRST build row of its key in      */
                              /* input order: unordered_map::insert, partitioned_hash.h:166-170   */
#define HMJ_CHECKSUM 0x08u    /* also fill xor_fold / mix_sum (parity checks)                     */
#define HMJ_SUM_PROBE 0x10u   /* also fill sum_probe_all (the 'miss inserts 0' sum of             */
                              /* hashjoin_bench.cc:92-96 is sum_probe_all + sum_r w/ FIRST_WINS)  */
#define HMJ_NULL_EQUAL 0x20u  /* NULL key slots compare equal to NULL slots of the same column     */
                              /* (IS NOT DISTINCT FROM): hmj_join_kind_cols_device and            */
                              /* hmj_join_mixed_device, see "NULL-equals-NULL matching" below     */

typedef struct {
  uint64_t n_matches;
  uint64_t sum_r;         /* sum of rval over result rows, mod 2^64                               */
  uint64_t sum_s;         /* sum of sval over result rows; sum_r + sum_s == hashjoin_bench.cc:132 */
  uint64_t xor_fold;      /* XOR over rows of tmix(key,rval,sval)        (HMJ_CHECKSUM)           */
  uint64_t mix_sum;       /* sum over rows of tmix(key,rval,sval)        (HMJ_CHECKSUM)           */
  uint64_t sum_probe_all; /* sum of val over ALL probe rows              (HMJ_SUM_PROBE)          */
  /* Result columns, n_matches entries each, NULL unless HMJ_MATERIALIZE.  Owned by the ctx,
   * valid until the next hmj_join_* / hmj_release_result / hmj_destroy on it.
   * hmj_join_u64_device: device pointers.  hmj_join_u64: host pointers.                       */
  const uint64_t* key;
  const uint64_t* rval;
  const uint64_t* sval;
} hmj_result;

/* Per-phase device time of the last join (HIP events on the ctx stream) and the algorithmic
 * bytes each phase moves (DESIGN.md "algorithmic bytes").  Valid after hmj_set_profiling(ctx,1). */
typedef struct {
  float ms_total;
  float ms_h2d, ms_d2h;           /* hmj_join_u64 only                                          */
  float ms_partition_build;       /* all radix passes over R                                    */
  float ms_partition_probe;       /* all radix passes over S                                    */
  float ms_hist, ms_scan, ms_scatter; /* the same time split by kernel kind (both relations)    */
  float ms_offsets;               /* partition boundary search                                  */
  float ms_probe_count;           /* build+probe kernel, count/sum mode                         */
  float ms_out_scan;              /* exclusive scan of per-partition match counts               */
  float ms_probe_write;           /* build+probe kernel, materialising mode                     */
  float ms_order;                 /* in-partition sort for HMJ_ORDERED                          */
  int radix_bits;                 /* total partition bits B (2^B partitions)                    */
  int radix_passes;               /* LSD passes per relation                                    */
  int n_scatter_launches;         /* scatter kernel launches in this join                       */
  int n_split_retries;            /* skewed joins: times the virtual-partition table was regrown        */
  uint64_t bytes_scatter;         /* algorithmic bytes of all scatter launches (32 B/tuple)     */
  uint64_t bytes_hist;            /* 16 B/tuple per pass                                        */
  uint64_t bytes_probe_count;     /* 16*(n_build + n_probe)                                     */
  uint64_t bytes_probe_write;     /* 16*(n_build + n_probe) + 24*n_matches                      */
  /* which code paths the last join took -- filled with or without profiling; the tests assert on these
   * instead of on wall-clock budgets                                                                */
  uint32_t path;                  /* HMJ_PATH_* bits                                            */
  int32_t key_prefix_bits;        /* top key bits skipped as shared by all rows (sampled or set)*/
  int32_t key_window_low;         /* lowest key bit of the B-bit partition window               */
  uint32_t n_probe_items;         /* probe work items: (virtual) partitions x probe slices      */
  float ms_scatter_pass[2];       /* ms_scatter split: [0] first radix pass of a relation (slab A),
                                     [1] later passes (slab B); both relations                  */
} hmj_timing;
#define HMJ_PATH_SLAB 0x001u           /* histogram-free slab partitioning                                */
#define HMJ_PATH_EXACT 0x002u          /* histogram + scan + scatter passes                               */
#define HMJ_PATH_UNIQ_WRITE 0x004u     /* materialised in one probe pass (unique build keys)              */
#define HMJ_PATH_SPLIT 0x008u          /* oversized partitions cut into virtual partitions                */
#define HMJ_PATH_WINDOW 0x010u         /* partition window moved below the shared prefix (structured keys)*/
#define HMJ_PATH_ORDER_DEFERRED 0x020u /* ordered epilogue finished by global LSD sorts of the result     */
#define HMJ_PATH_ORDER_BY_KEY 0x040u   /* partitions are not key ranges: final stable sort by key         */
#define HMJ_PATH_PREPARED 0x080u       /* build side taken from hmj_prepare_build_u64_device              */
#define HMJ_PATH_CHUNKED_BUILD 0x100u  /* plan with build partitions beyond the LDS table (forced bits)   */
#define HMJ_PATH_HOT_KEY_HINT 0x200u   /* the key sample saw a repeated key                               */
#define HMJ_PATH_SLAB_PROBE 0x400u     /* probe-heavy count join: build side exact, probe side in slabs   */
#define HMJ_PATH_SORTED_WRITE 0x800u   /* ordered join probed, sorted and written in one pass             */
#define HMJ_PATH_SORTED_FK 0x1000u     /* ... in its foreign-key form (probe keys repeat)                 */
#define HMJ_PATH_DENSE_BUILD 0x2000u   /* build keys cover part of the key range: plan sized by their density */
#define HMJ_PATH_SORTED_FK_HALF 0x8000u /* ... in its small shape: 512-thread workgroups, two per CU                */
#define HMJ_PATH_SORTED_FK_WIDE 0x20000u /* ... in its wide shape: 6144 probe rows per partition (16-bit plan, slab path)    */
#define HMJ_PATH_LOOKBACK_TIMEOUT 0x10000u /* a chained partition gave up waiting for its predecessor (a bug if seen) */
#define HMJ_PATH_PRESORTED 0x40000u /* a relation arrived already partitioned (sorted by key): its radix passes were skipped */
#define HMJ_PATH_SLAB_ONE_PASS 0x80000u /* ... of a ONE-pass plan: the probe kernel reads the pass's worker-private slabs directly */
#define HMJ_PATH_ORDER_BY_RANK_SORT 0x200000u /* ordered, small build side under a long probe side: rows sorted as (key rank, payload) composites */
#define HMJ_PATH_RANK_RUNS 0x1000000u /* ... rows partitioned by key rank -- longer runs: by (rank, piece of the payloads' range) -- with two slab passes, each partition sorted in LDS */
#define HMJ_PATH_RANK_LOOKUP_IN_PASS 0x2000000u /* ... with the key -> rank lookup inside the first slab pass (every probe row had its build row) */
#define HMJ_PATH_SORT_MSD 0x4000000u /* hmj_sort_u64_device: two slab passes on the top varying key bits + an LDS sort of every partition */
#define HMJ_PATH_KEY_RANGES 0x8000000u /* ordered join no single plan holds: both relations cut into key ranges, joined one after the other, rows appended */
#define HMJ_PATH_ORDERED_EXPANSION 0x400000u /* ordered, duplicate build keys: rows written in order partition by partition (no sort of result rows) */
#define HMJ_PATH_LDS_TABLE 0x800000u /* ... of <= 2048 build rows (1024 with HMJ_CHECKSUM / HMJ_SUM_PROBE) under >= 2^16 probe rows, count modes: that table in LDS, one copy per workgroup */
#define HMJ_PATH_GLOBAL_TABLE 0x100000u /* small build side: one global hash table, the probe side streamed unpartitioned */
#define HMJ_PATH_HOST_PIPELINE 0x4000u /* host entry: build side partitioned while the probe side was uploading   */
#define HMJ_PATH_PROBE_KEYS 0x10000000u /* plain count join on the slab path whose probe side went through the passes as 8-byte KEYS:
                                          every probe row met exactly one build row (verified by the probe kernel), so sum_s is the
                                          sum of all probe payloads, added up by pass A.  Set only when the result came from that form */

/* How the last join on this ctx was planned, and why (hmj_last_plan).  The planner chooses among the formulations listed
 * at hmj_join_u64_device from the sizes, the flags, a key sample and what EARLIER JOINS OF THE SAME WORKLOAD taught it:
 * a fast path that gives up (a slab overflowed on skewed keys, the unique-key write met duplicate build keys, the global
 * table's walk got too long) is retried on the general path within the same join and then skipped for the next 8 (64)
 * joins of that workload.  A workload = floor(log2) of both sizes + the mode flags (materialise / ordered / first-wins);
 * joins of other shapes on the same ctx are not affected (round 5; until then the cool-downs belonged to the ctx).
 * Tests assert on these fields instead of pinning paths through the environment.  Nothing in the reference corresponds
 * (its one plan is optimal_partition, radix_hash.h:38-57).                                                         */
typedef struct {
  uint32_t struct_size;   /* bytes the library filled in (callers built against an older header get a prefix)      */
  uint32_t path;          /* HMJ_PATH_* of the attempt that produced the result (= hmj_timing.path)                */
  int32_t radix_bits, radix_passes, pass_bits[4];
  int32_t key_prefix_bits, key_window_low;
  uint32_t n_partitions;  /* 2^radix_bits, or 0 where nothing was partitioned (global / LDS table)                 */
  uint32_t probe_items;   /* work items of the probe phase ((virtual) partitions x probe slices)                   */
  uint32_t attempts;      /* plans executed for this join (1 = the first plan held)                                */
  uint32_t refused;       /* HMJ_REFUSED_*: faster formulations not taken by this join, and why                    */
  uint32_t cooling;       /* HMJ_COOL_*: fast paths this WORKLOAD is skipping after this join (0 = nothing learnt) */
  uint64_t workload;      /* the signature the adaptive state is keyed by                                          */
} hmj_plan_desc;
#define HMJ_REFUSED_GTABLE_SHAPE 0x0001u        /* global table: build side / flags / sizes outside its window          */
#define HMJ_REFUSED_GTABLE_COOLING 0x0002u      /* ... skipped: an earlier join of this workload gave up on it          */
#define HMJ_REFUSED_GTABLE_GAVE_UP 0x0004u      /* ... tried by THIS join and abandoned (duplicate keys, long walks)     */
#define HMJ_REFUSED_RANK_SORT_MODEL 0x0008u     /* ordered small build side: the cost model preferred partitioning       */
#define HMJ_REFUSED_RANK_SORT_COOLING 0x0010u
#define HMJ_REFUSED_RANK_SORT_GAVE_UP 0x0020u
#define HMJ_REFUSED_SLAB_SHAPE 0x0040u          /* slab partitioning: not a two-pass plan of <= 9-bit passes, sizes below */
                                                /* the threshold, or probe partitions beyond the pipelined kernels        */
#define HMJ_REFUSED_SLAB_COOLING 0x0080u
#define HMJ_REFUSED_SLAB_SORTED_INPUT 0x0100u   /* the sample found a relation in key order (its digits are not mixed)   */
#define HMJ_REFUSED_SLAB_OVERFLOW 0x0200u       /* tried by this join: a slab overflowed (skewed digits), exact passes    */
#define HMJ_REFUSED_FAST_WRITE_COOLING 0x0400u  /* unique-key write mode skipped: duplicate build keys seen earlier       */
#define HMJ_REFUSED_FAST_WRITE_GAVE_UP 0x0800u  /* ... tried by this join: duplicate build keys / an oversized partition  */
#define HMJ_REFUSED_SLAB_PROBE_COOLING 0x1000u  /* probe-side-only slabs / one-pass slab walk skipped                     */
#define HMJ_REFUSED_SLAB_PROBE_OVERFLOW 0x2000u
#define HMJ_REFUSED_PREFIX_VIOLATED 0x4000u     /* a row outside the sampled key prefix: the join re-planned              */
#define HMJ_REFUSED_EXPANSION_GAVE_UP 0x8000u   /* ordered expansion: a partition beyond the kernel's capacity            */
#define HMJ_REFUSED_PROBE_KEYS_GAVE_UP 0x10000u /* key-only probe side tried by this join: a probe row without exactly one  */
                                                /* build row; the probe side was redone with whole rows (build slabs kept)  */
#define HMJ_REFUSED_PROBE_KEYS_COOLING 0x20000u /* ... skipped: an earlier join of this workload gave up on it             */
#define HMJ_COOL_UNIQ_WRITE 0x001u
#define HMJ_COOL_SORTED_WRITE 0x002u
#define HMJ_COOL_GTABLE 0x004u
#define HMJ_COOL_GTABLE_WRITE 0x008u
#define HMJ_COOL_RANK_SORT 0x010u
#define HMJ_COOL_RANK_SORT_SLAB 0x020u
#define HMJ_COOL_EXPANSION 0x040u
#define HMJ_COOL_SORT_SLAB 0x080u
#define HMJ_COOL_SLAB 0x100u
#define HMJ_COOL_SLAB_PROBE 0x200u
#define HMJ_COOL_ONE_PASS_WRITE 0x400u
#define HMJ_COOL_EXACT_PREFIX 0x800u
#define HMJ_COOL_RANK_RUNS 0x1000u
#define HMJ_COOL_SORT_MSD 0x2000u
#define HMJ_COOL_PROBE_KEYS 0x4000u

/* ---- lifecycle ------------------------------------------------------------------------------- */
/* Replaces: nothing in the reference (no device); one ctx per GPU. device_id < 0 = current.     */
int hmj_create(hmj_ctx** out, int device_id);
void hmj_destroy(hmj_ctx* ctx);
/* Launch on the caller's HIP stream (hipStream_t passed as void*).  NULL is the HIP default (null)
 * stream, exactly as in the HIP API; HMJ_STREAM_OWN selects the ctx's private non-blocking stream
 * (the initial setting).  Device inputs must be complete on, or ordered before, the chosen stream:
 * the private stream does NOT synchronise with work queued on other streams.                      */
#define HMJ_STREAM_OWN ((void*)(intptr_t)-1)
int hmj_set_stream(hmj_ctx* ctx, void* hip_stream);
/* Pre-allocate workspace for joins up to these sizes (so the timed call allocates nothing).     */
int hmj_reserve(hmj_ctx* ctx, uint64_t n_build, uint64_t n_probe, uint64_t max_matches,
                uint32_t flags);
/* Override the planner (the reference's optimal_partition heuristic, radix_hash.h:38-57, is tuned
 * for CPU caches; ours targets LDS capacity).  total_bits < 0 restores automatic planning.       */
int hmj_set_radix_bits(hmj_ctx* ctx, int total_bits);
/* Measure the plan instead of trusting the heuristic (the reference tunes its k with
 * find_k_bench.cc:116-129): joins synthetic relations of the given sizes (unique uniform keys, every
 * probe row matching once -- the hmj_gen_* generators) with B-1, B and B+1 total radix bits, B being
 * hmj_plan's choice, and reports the time of each (ms[0..2]; a candidate that does not exist is < 0).
 * apply != 0 keeps the fastest as the forced plan of this ctx (as hmj_set_radix_bits would).  Needs
 * 16*(n_build+n_probe) bytes of device memory beside the join's workspace.                         */
int hmj_autotune_radix_bits(hmj_ctx* ctx, uint64_t n_build, uint64_t n_probe, int apply, int* best_bits,
                            double ms[3]);
/* Tell the executor that the top `bits` key bits are equal in all rows of both relations (an outer
 * radix split of the caller's already consumed them; hmj_exchange_join_u64_device needs none): partitioning then starts
 * below them, as the reference's recursion masks off consumed bits (radix_hash.h:219-220).
 * bits = -1 (the default): the executor samples both relations and skips the top bits all sampled
 * keys share (dense / small-integer keys would otherwise all fall into partition 0).
 * Any value is safe for the counts, the sums and the set of result rows (every window of key bits is a
 * partition function).  The ORDER of HMJ_ORDERED output relies on partitions being key ranges: a sampled
 * prefix is verified on every row, and the join re-plans without it if a row disagrees; a prefix given
 * here is the caller's promise and is taken as it is.
 * The hint describes the caller's u64 relations -- hmj_join_u64_device, the u64 kind entries, the host and
 * exchange joins.  The string, multi-column and mixed-key entries join on a key64 of their own (a hash, or
 * a packed tuple): their internal joins always sample that key64 and never read the hint, and they leave
 * it in place for the caller's next u64 join.                                                    */
int hmj_set_key_prefix_bits(hmj_ctx* ctx, int bits);
/* The automatic plan for a build side of n_build rows: total bits and per-pass bits (LSD order).*/
int hmj_plan(uint64_t n_build, int* total_bits, int* n_passes, int pass_bits[4]);
/* Placement of the big partition buffers (how fast a buffer can be written is a property of the
 * physical memory behind it).  Every partition buffer of 2 GiB and more is probed when it is created (two fills, the
 * second timed: ~2.4 ms for 6 GB).  A SEARCH for faster memory -- further candidate allocations, the fastest kept --
 * runs only inside hmj_reserve (the caller asked for the workspace ahead of time) or when HMJ_PLACE=n is set in the
 * environment; a join that allocates on its own never searches.  A search keeps at most two candidates alive, tries
 * at most n (default 4) and stops when its wall-clock budget (HMJ_PLACE_BUDGET_MS, default 50 ms per buffer) would be
 * exceeded.  HMJ_PLACE=0: nothing is probed.  One entry per probed buffer of this ctx; returns the number of entries
 * (<= max_entries).  Diagnostic only; nothing in the reference corresponds to it (its buffers are std::vector
 * storage, hashjoin.h:62-63).                                                                                    */
/* hmj_place_info, hmj_timing and hmj_exchange_info are DIAGNOSTIC structs: they grow between releases of this library and
 * carry no size field -- build callers against the header of the library they load (hmj_abi_version() == HMJ_ABI_VERSION).
 * hmj_plan_desc, added later, is size-versioned instead.                                                              */
#define HMJ_ABI_VERSION 5
int hmj_abi_version(void);
#define HMJ_PLACE_MAX_CAND 4
typedef struct {
  char name[16];      /* slab_a, slab_b_build, slab_b_probe, rbuf0/1, sbuf0/1                                   */
  uint64_t bytes;
  float fill_TBps;    /* of the allocation that was kept: second of two sequential fills                         */
  int candidates;     /* allocations tried (1 = the first one was kept without a search)                         */
  float ms_search;    /* host time of probe(s) and search, part of the call that allocated the buffer            */
  int searched;       /* 1: a search was allowed (hmj_reserve / HMJ_PLACE=n); 0: probe only                      */
  int aborted;        /* 1: the search stopped because its budget was reached                                    */
  float budget_ms;
  float cand_ms_alloc[HMJ_PLACE_MAX_CAND]; /* per candidate: hipMalloc                                           */
  float cand_ms_fill[HMJ_PLACE_MAX_CAND];  /* per candidate: the two fills (+ the loser's hipFree)               */
  float cand_TBps[HMJ_PLACE_MAX_CAND];     /* per candidate: fill rate                                           */
} hmj_place_info;
int hmj_placement_info(hmj_ctx* ctx, hmj_place_info* out, int max_entries);
/* out->struct_size must hold sizeof(hmj_plan_desc) of the CALLER's header on entry; at most that many bytes are written. */
int hmj_last_plan(hmj_ctx* ctx, hmj_plan_desc* out);
/* Forget what the ctx has learnt about every workload (all cool-downs, the ordered kernels' adaptive forms).          */
int hmj_forget_workloads(hmj_ctx* ctx);
int hmj_set_profiling(hmj_ctx* ctx, int enabled);
int hmj_last_timing(hmj_ctx* ctx, hmj_timing* out);
const char* hmj_strerror(int code);
const char* hmj_last_error(hmj_ctx* ctx);
const char* hmj_version(void);

/* ---- the join ---------------------------------------------------------------------------------- */
/* Replaces HashMergeJoin<RIter,SIter>::HashMergeJoin(r_begin,r_end,s_begin,s_end,num_threads)
 * (hashjoin.h:56-68) plus the iteration that consumes it (hashjoin.h:183-191, driven as in
 * hashjoin_bench.cc:126-133), and equally the partition_only + partitioned_hash_table + probe loop
 * of hashjoin_bench.cc:88-96 (partitioned_hash.h:82-124, :173-215).
 * Inputs are device-resident, borrowed, read-only, not retained after return.  Blocking: on
 * return `out` is filled and the result columns are complete on the stream.
 * Which formulation runs is the executor's choice (hmj_timing.path says which; results are the same):
 *   - two radix passes + LDS build/probe per partition (the default from ~2^21 rows per side on; histogram-free slab
 *     passes of up to 9 bits, so up to 2^30 rows per side stay at 32 B per row and pass);
 *   - ... flags = 0, >= 2^25 probe rows, passes of <= 8 bits, and EVERY probe row meets exactly one build row (a foreign key
 *     into a unique dimension key): the probe side goes through the slab passes as 8-byte keys -- 48 instead of 80 bytes per
 *     probe row -- while its first pass adds up the payloads, which then ARE sum_s; HMJ_PATH_PROBE_KEYS.  A pilot over 4096
 *     sampled probe rows decides whether a workload's first join starts that way, the probe kernel verifies every probe
 *     row's match count, and a join that fails the check redoes its probe side with whole rows inside the same plan
 *     (HMJ_REFUSED_PROBE_KEYS_GAVE_UP; the workload then keeps whole rows for 8 joins, HMJ_COOL_PROBE_KEYS);
 *   - count modes and unordered HMJ_MATERIALIZE, build side of <= 2^17 rows (or a join of <= 2^21 rows in all): ONE global
 *     hash table, the probe side streamed unpartitioned -- the reference's BM_hash_join_raw formulation
 *     (hashjoin_bench.cc:29-63), HMJ_PATH_GLOBAL_TABLE (count modes, <= 2048 build rows: the table in LDS, HMJ_PATH_LDS_TABLE);
 *   - the same modes, build side of 2^17 ... 2^21 rows under a probe side >= 8 x larger: one radix pass, the probe side left
 *     in the worker-private slabs of its slab pass and probed there, HMJ_PATH_SLAB_ONE_PASS;
 *   - HMJ_ORDERED, small build side under a probe side >= 128 x larger (a cost model over fan-out and size decides): the
 *     rows ordered through the RANK of their key among the sorted build keys, HMJ_PATH_ORDER_BY_RANK_SORT -- partitioned
 *     by rank (runs beyond ~1700 rows: by rank and the position of the payload in the payloads' range), every partition
 *     sorted in LDS (HMJ_PATH_RANK_RUNS); where that does not apply (more than 2^18 partitions, probe rows without a
 *     build row in a cut run, a hot key): (rank, payload) composites sorted by global LSD passes.
 * hmj_last_plan says which was taken and why the faster ones were not.                                               */
int hmj_join_u64_device(hmj_ctx* ctx, const void* build_aos_dev, uint64_t n_build,
                        const void* probe_aos_dev, uint64_t n_probe, uint32_t flags,
                        hmj_result* out);
/* Join kinds other than the inner join: for each PROBE row, by whether its key occurs on the build side.
 *   HMJ_JOIN_SEMI        each probe row with >= 1 build row of its key, once (EXISTS / IN (subquery));
 *   HMJ_JOIN_ANTI        each probe row with no build row of its key (NOT EXISTS);
 *   HMJ_JOIN_PROBE_OUTER the inner rows + one (key, outer_fill, sval) row per unmatched probe row.  With HMJ_FIRST_WINS and
 *                        outer_fill = 0 this is, row by row, the reference's partitioned probe loop (hashjoin_bench.cc:92-96:
 *                        r.second + s_tables[i][r.first], operator[] yielding 0 on a miss).
 * Result columns: SEMI / ANTI produce key and sval (rval is NULL); PROBE_OUTER all three.  Row order is unspecified without
 * HMJ_ORDERED; with it rows are sorted ascending by (key, rval, sval), or (key, sval) for SEMI / ANTI.
 * Duplicate probe keys are independent rows.  Duplicate build keys: SEMI emits a probe row once however many partners it
 * has; PROBE_OUTER pairs it with all of them (with the first only, under HMJ_FIRST_WINS); HMJ_FIRST_WINS does not change
 * SEMI / ANTI.  n_matches = result rows; sum_r / sum_s and HMJ_CHECKSUM's tmix(key, rval, sval) are taken over result rows
 * with rval = 0 for SEMI / ANTI rows and rval = outer_fill for unmatched outer rows; HMJ_SUM_PROBE is unchanged.
 * n_build == 0: ANTI returns the whole probe side, PROBE_OUTER every probe row with the fill.
 * kind == HMJ_JOIN_INNER: exactly hmj_join_u64_device (path, result, timing); the two counters are not filled.
 * HMJ_E_ARG: NULL ctx / opts / out, opts->struct_size too small for kind and outer_fill, an unknown kind, more than 2^32-1
 * rows.  HMJ_E_UNSUPPORTED wherever the inner ordered join returns it.  Like any other call it discards a prepared build
 * side.  The planner takes only plans whose probe phase is the partition-by-partition walk (DESIGN.md "Join kinds"): no
 * global / LDS table, one-pass slab walk, unique-key / sorted writes, rank forms, ordered expansion or key ranges, and no
 * build partition is cut into build slices.  Nothing in the reference's operator corresponds (it has no join kinds).     */
#define HMJ_JOIN_INNER 0u       /* = hmj_join_u64_device                                                  */
#define HMJ_JOIN_SEMI 1u        /* each probe row with >= 1 build row of its key, once                     */
#define HMJ_JOIN_ANTI 2u        /* each probe row with no build row of its key                             */
#define HMJ_JOIN_PROBE_OUTER 3u /* inner rows + one (key, outer_fill, sval) row per unmatched probe row     */
typedef struct {
  uint32_t struct_size;       /* in: sizeof(hmj_join_opts) of the caller's header (size-versioned like hmj_plan_desc) */
  uint32_t kind;              /* in: HMJ_JOIN_*                                                                      */
  uint64_t outer_fill;        /* in: rval of an unmatched probe row; 0 = the reference's operator[] default          */
  uint64_t n_probe_matched;   /* out: probe rows with >= 1 build partner (kinds other than INNER)                     */
  uint64_t n_probe_unmatched; /* out: n_probe - n_probe_matched                                                      */
} hmj_join_opts;
int hmj_join_kind_u64_device(hmj_ctx* ctx, const void* build_aos_dev, uint64_t n_build,
                             const void* probe_aos_dev, uint64_t n_probe, uint32_t flags,
                             hmj_join_opts* opts, hmj_result* out);
/* Join kinds that answer for each BUILD row whether its key occurs on the probe side, and the full outer join:
 *   HMJ_BUILD_SEMI  each build row with >= 1 probe row of its key, once (right semi join);
 *   HMJ_BUILD_ANTI  each build row with no probe row of its key (right anti join);
 *   HMJ_BUILD_OUTER the inner rows + one (key, rval, build_fill) row per unmatched build row (right outer join);
 *   HMJ_FULL_OUTER  the inner rows + one (key, probe_fill, sval) row per unmatched probe row + one (key, rval, build_fill)
 *                   row per unmatched build row -- in one call, where composing it takes two joins.
 * A build row is matched when its key occurs on the probe side; duplicate build rows are independent rows (each is emitted
 * by BUILD_SEMI / BUILD_ANTI at most once, however many probe partners it has).  The pair rows of BUILD_OUTER / FULL_OUTER
 * are exactly the inner join's: every probe row with every build row of its key.  HMJ_FIRST_WINS does not change
 * BUILD_SEMI / BUILD_ANTI and is HMJ_E_ARG with the outer kinds (a non-first duplicate build row would be neither paired
 * nor unmatched).  Result columns: BUILD_SEMI / BUILD_ANTI produce key and rval (sval is NULL); the outer kinds all three.
 * Row order is unspecified without HMJ_ORDERED; with it rows are sorted ascending by (key, rval, sval), or (key, rval) for
 * BUILD_SEMI / BUILD_ANTI.  n_matches = result rows; sum_r / sum_s and HMJ_CHECKSUM's tmix(key, rval, sval) are taken over
 * result rows with sval = 0 for build semi / anti rows, sval = build_fill for unmatched build rows and rval = probe_fill for
 * unmatched probe rows; HMJ_SUM_PROBE is unchanged.  n_probe == 0: BUILD_ANTI, BUILD_OUTER and FULL_OUTER return every
 * build row; n_build == 0: FULL_OUTER returns every probe row with the fill.
 * HMJ_E_ARG: NULL ctx / opts / out, opts->struct_size too small for the fields the kind reads, an unknown kind, more than
 * 2^32-1 rows per side.  HMJ_E_UNSUPPORTED wherever the kind joins return it.  Like any other call it discards a prepared
 * build side.  Plans as hmj_join_kind_u64_device's (DESIGN.md "Join kinds"): the probe walk marks, in one bit per build row,
 * the rows whose key a probe row met, and a sweep over the partitioned build side emits build rows by that mark.       */
#define HMJ_BUILD_SEMI 1u  /* each build row with >= 1 probe row of its key, once          -> (key, rval)          */
#define HMJ_BUILD_ANTI 2u  /* each build row with no probe row of its key                   -> (key, rval)          */
#define HMJ_BUILD_OUTER 3u /* inner rows + one (key, rval, build_fill) per unmatched build row                     */
#define HMJ_FULL_OUTER 4u  /* inner rows + (key, probe_fill, sval) per unmatched probe row
                                       + (key, rval, build_fill) per unmatched build row                         */
typedef struct {
  uint32_t struct_size;       /* in: sizeof(hmj_build_join_opts) of the caller's header (size-versioned like hmj_join_opts) */
  uint32_t kind;              /* in: HMJ_BUILD_SEMI / _ANTI / _OUTER / HMJ_FULL_OUTER                                    */
  uint64_t build_fill;        /* in: sval of an unmatched build row (BUILD_OUTER, FULL_OUTER)                            */
  uint64_t probe_fill;        /* in: rval of an unmatched probe row (FULL_OUTER)                                         */
  uint64_t n_build_matched;   /* out: build rows with >= 1 probe partner                                                 */
  uint64_t n_build_unmatched; /* out: n_build - n_build_matched                                                          */
  uint64_t n_probe_matched;   /* out: FULL_OUTER only (0 otherwise)                                                      */
  uint64_t n_probe_unmatched; /* out: FULL_OUTER only (0 otherwise)                                                      */
} hmj_build_join_opts;
int hmj_join_build_kind_u64_device(hmj_ctx* ctx, const void* build_aos_dev, uint64_t n_build,
                                   const void* probe_aos_dev, uint64_t n_probe, uint32_t flags,
                                   hmj_build_join_opts* opts, hmj_result* out);
/* The join kinds of both families across ranks: the collective counterpart of the two entries above, on row shards as
 * hmj_exchange_join_u64_device takes them (multi-GPU section below: communicator, owners, rounds, errors).
 * opts->side selects the family: HMJ_KIND_PROBE_SIDE with kind HMJ_JOIN_INNER / _SEMI / _ANTI / _PROBE_OUTER, or
 * HMJ_KIND_BUILD_SIDE with HMJ_BUILD_SEMI / _ANTI / _OUTER / HMJ_FULL_OUTER.  Each kind means what it means on one GPU --
 * result columns, fill rules, sums and checksums over result rows, HMJ_SUM_PROBE, what an empty side returns -- with the
 * relations being the union of every rank's shards.  The exchange gives every key's rows of both relations to one owner
 * rank; each rank runs the single-GPU kind join on what it owns (per digit round of the digit-owner path, or once on the
 * owner-split path), so a probe row without a partner in its own rank's build shard is answered against the whole build side.
 *   local_out  this rank's rows and sums for the keys it owns (materialising flags: device columns owned by the ctx);
 *   global_out (may be NULL) the sums over all ranks, columns NULL -- as for the inner exchange join;
 *   opts->local / opts->global  the counters the single-GPU entry of the kind fills (probe counters for SEMI / ANTI /
 *              PROBE_OUTER, build counters for the build kinds, both for FULL_OUTER), zeros where a kind defines none;
 *              local over the rows this rank received, global summed over the ranks.
 * HMJ_ORDERED: each rank's rows are sorted as on one GPU and, concatenated in rank order, are the global order (key-range
 * owners).  HMJ_FIRST_WINS with PROBE_OUTER is global first-wins under the inner exchange join's rule: rank r's build
 * shard precedes rank r+1's.  HMJ_KIND_PROBE_SIDE + HMJ_JOIN_INNER is exactly hmj_exchange_join_u64_device (counters 0).
 * Collective: every rank passes the same flags, side and kind.  HMJ_E_ARG at once, on every rank alike: NULL ctx / opts /
 * local_out, opts->struct_size too small for the fields the kind reads, an unknown side or kind, HMJ_FIRST_WINS with
 * BUILD_OUTER or FULL_OUTER.  A rank's own errors travel to the final reduction and all ranks return together; ranks that
 * disagree on (side, kind) all return HMJ_E_ARG there.                                                                  */
#define HMJ_KIND_PROBE_SIDE 0u /* kind is HMJ_JOIN_INNER / _SEMI / _ANTI / _PROBE_OUTER                                  */
#define HMJ_KIND_BUILD_SIDE 1u /* kind is HMJ_BUILD_SEMI / _ANTI / _OUTER or HMJ_FULL_OUTER                              */
typedef struct {
  uint64_t n_probe_matched, n_probe_unmatched, n_build_matched, n_build_unmatched;
} hmj_kind_counts;
typedef struct {
  uint32_t struct_size;   /* in: sizeof(hmj_exchange_kind_opts) of the caller's header                                  */
  uint32_t side;          /* in: HMJ_KIND_PROBE_SIDE / HMJ_KIND_BUILD_SIDE                                              */
  uint32_t kind;          /* in: a kind of that side                                                                    */
  uint32_t reserved;      /* in: 0                                                                                      */
  uint64_t probe_fill;    /* in: rval of an unmatched probe row (PROBE_OUTER, FULL_OUTER)                               */
  uint64_t build_fill;    /* in: sval of an unmatched build row (BUILD_OUTER, FULL_OUTER)                               */
  hmj_kind_counts local;  /* out: over the rows this rank received (the keys it owns)                                   */
  hmj_kind_counts global; /* out: summed over all ranks                                                                 */
} hmj_exchange_kind_opts;
int hmj_exchange_join_kind_u64_device(hmj_ctx* ctx, const void* build_shard_dev, uint64_t n_build_shard,
                                      const void* probe_shard_dev, uint64_t n_probe_shard, uint32_t flags,
                                      hmj_exchange_kind_opts* opts, hmj_result* local_out, hmj_result* global_out);
/* Partition the build side ahead of the join (e.g. while the probe side is still arriving over
 * xGMI).  One-shot: the NEXT hmj_join_u64_device on this ctx whose build pointer, row count and plan
 * match (count modes and materialising joins of relations of similar size plan alike; a join that plans
 * differently simply partitions R again) skips re-partitioning R; any other call discards the prepared state.  The caller promises the build rows do not change in between.
 * "Any other call" is every call that runs on the device or touches the workspace: the joins of every kind (u64, string,
 * multi-column -- hmj_join_cols_device, hmj_join_kind_cols_device --, mixed-key -- hmj_join_mixed_device --, host-resident, exchange), hmj_sort_u64_device, hmj_sort_rows_by_u64_host, hmj_argsort_u64_host, hmj_partition_u64_device,
 * hmj_hash_str_device (each of them also when given no rows), hmj_top_k_device (where it has entries to return), hmj_reserve and hmj_autotune_radix_bits.  Left out are the calls that read or write no workspace buffer: hmj_set_stream,
 * hmj_set_radix_bits / hmj_set_key_prefix_bits (the join then plans other bits and partitions R again), hmj_set_profiling,
 * hmj_forget_workloads, hmj_release_result (result columns only), the hmj_last_* / hmj_placement_info queries, the
 * hmj_gen_* generators, hmj_take_cols_device and hmj_take_str_device (their only workspace is small buffers of their own); a call refused with HMJ_E_ARG before it started may leave the prepared state in place as well.
 * n_probe_hint: the probe size the join will have (it selects the partitioning path).
 * Corresponds to the first radix_non_inplace_par call of the reference ctor (hashjoin.h:65).       */
int hmj_prepare_build_u64_device(hmj_ctx* ctx, const void* build_aos_dev, uint64_t n_build,
                                 uint64_t n_probe_hint);
/* Same with host-resident relations (what a caller of the reference's ctor holds: pointers into
 * std::vector<std::pair<uint64_t,uint64_t>>).  Copies in over PCIe, joins, copies results out.   */
int hmj_join_u64(hmj_ctx* ctx, const void* build_aos_host, uint64_t n_build,
                 const void* probe_aos_host, uint64_t n_probe, uint32_t flags, hmj_result* out);
void hmj_release_result(hmj_ctx* ctx);

/* Host-resident join whose result columns are DETACHED from the ctx: *rows owns the three
 * host columns (out->key/rval/sval point into them) until hmj_rows_free, independent of later joins
 * on the ctx or of the ctx's lifetime -- the ownership HashMergeJoin's _r_sorted/_s_sorted vectors
 * have in the reference (hashjoin.h:197-198).  Freed buffers return to a process-wide pool of
 * huge-page host memory, so a construct/clear loop like hashjoin_bench.cc:120-134 does not fault its
 * result memory in again every iteration.
 * Implies HMJ_MATERIALIZE.  hmj_rows_free(NULL) is a no-op; it may be called from any thread.     */
typedef struct hmj_rows hmj_rows;
int hmj_join_u64_rows(hmj_ctx* ctx, const void* build_aos_host, uint64_t n_build,
                      const void* probe_aos_host, uint64_t n_probe, uint32_t flags, hmj_result* out,
                      hmj_rows** rows);
void hmj_rows_free(hmj_rows* rows);
/* Released result columns and staging slots return to a process-wide pool of host memory that keeps at
 * most HMJ_HOST_POOL_MAX_MB (environment, default 8192) MiB; beyond that the oldest buffers go back to the
 * OS.  hmj_host_pool_trim(keep) shrinks the pool to at most `keep` bytes now (0 empties it) and returns the
 * bytes released; hmj_host_pool_bytes() reports what the pool holds.  Both are thread-safe.  (The
 * reference frees its _r_sorted/_s_sorted vectors in clear(), hashjoin.h:192-195.)                     */
uint64_t hmj_host_pool_trim(uint64_t keep_bytes);
uint64_t hmj_host_pool_bytes(void);

/* ---- string keys on the device ------------------------------------------------------------------ */
/* Replaces HashMergeJoin<KeyValVec::iterator, KeyValVec::iterator> (hashjoin.h:29 KeyValVec = pair<std::string,
 * uint64_t>, driven as hashjoin_bench.cc:109-143 drives it) for relations whose keys are variable-length byte strings
 * held on the device.  Relation layout: Arrow large_string / large_binary -- n + 1 64-bit offsets into one byte buffer --
 * plus a payload column.  Hashing, the join, key verification, payload gather and ordering all run on the GPU; no pass
 * on the host touches keys or rows.  (The C++ drop-in, hashmergejoin_hip.hpp, hashes on the host and is unchanged.)    */
typedef struct {
  const void* chars;        /* device: key bytes of all rows; may be NULL when every key is empty                  */
  const uint64_t* offsets;  /* device: n + 1 non-decreasing byte offsets; row i = chars[offsets[i], offsets[i+1])  */
                            /* offsets[0] need not be 0 (Arrow slices); chars need not be aligned                   */
  const uint64_t* vals;     /* device: n payloads (the reference's RValue / SValue)                                 */
  uint64_t n;               /* rows, <= 2^32 - 1                                                                    */
} hmj_str_rel;

/* std::hash<std::string> of every row (libstdc++'s _Hash_bytes, seed 0xc70f6907; other standard libraries hash
 * differently), on the device.  hash_bits 0 = all 64 bits; 1..63 = h >> (64 - hash_bits) (see hmj_str_join_opts).
 * hash_out_dev: n uint64 (device).  HMJ_E_ARG: NULL ctx, NULL offsets / hash_out_dev with n > 0, more than 2^32-1 rows,
 * hash_bits > 63, decreasing offsets (hmj_last_error names the first offending row), key bytes with chars == NULL.      */
int hmj_hash_str_device(hmj_ctx* ctx, const void* chars, const uint64_t* offsets, uint64_t n, uint32_t hash_bits,
                        uint64_t* hash_out_dev);

typedef struct {
  uint32_t struct_size;   /* in: sizeof of the caller's header (size-versioned like hmj_join_opts)                  */
  uint32_t hash_bits;     /* in: 0 = 64; fewer bits make hash collisions between different keys common --            */
                          /* exists so callers and tests can exercise collision handling                             */
  uint64_t n_hash_pairs;  /* out: pairs of equal hash the {hash,row} join produced                                   */
  uint64_t n_collisions;  /* out: of those, pairs whose keys differ (dropped)                                         */
  float ms_hash, ms_join, ms_verify, ms_order; /* out, with hmj_set_profiling(ctx, 1): HIP-event phase times          */
} hmj_str_join_opts;

typedef struct {
  uint64_t n_matches, sum_r, sum_s, xor_fold, mix_sum, sum_probe_all; /* as hmj_result; tmix over (hash, rval, sval) */
  const uint64_t *hash, *r_row, *s_row, *rval, *sval; /* HMJ_MATERIALIZE: device columns owned by the ctx, valid   */
                                                      /* until the next call on it / hmj_release_result            */
} hmj_str_result;

/* The inner equi-join of two string-keyed relations.
 * Match rule: a result row is a pair (build row, probe row) whose keys are equal byte for byte -- equal length and equal
 * bytes; embedded NUL bytes and bytes >= 0x80 are ordinary bytes.  Duplicate keys on either side give the cross product.
 * Row contents: r_row / s_row are row indices into the caller's relations (gather maps); rval = build->vals[r_row],
 * sval = probe->vals[s_row]; hash is the key's hash (hash_bits applied).
 * Flags: HMJ_MATERIALIZE, HMJ_ORDERED, HMJ_CHECKSUM and HMJ_SUM_PROBE mean what they mean for hmj_join_u64_device;
 * HMJ_FIRST_WINS is HMJ_E_ARG.  Without HMJ_MATERIALIZE only the counters and sums are filled; verification still runs,
 * so every count is exact.
 * HMJ_ORDERED: rows ascending by (hash, key bytes compared as std::string::operator< compares them, r_row, s_row).  For
 * keys unique within each relation this is exactly the reference operator's iteration order: ascending std::hash, ties
 * broken on the key (radix_hash.h:86-109).
 * How: every key is hashed into a {hash, row} row (str_hash_kernel; the wave's 64 keys staged in LDS), the two row sets
 * are joined by the u64 join (HMJ_MATERIALIZE, + HMJ_ORDERED), every pair of equal hash has its keys compared and its
 * payloads gathered (verify_kernel; survivors compacted stably), and -- ordered only -- runs of equal hash whose
 * build keys differ are sorted by key bytes, each inside one workgroup.
 * n == 0 on either side: an empty result and HMJ_OK.
 * HMJ_E_ARG: NULL ctx / rel / opts / out; NULL offsets or vals with n > 0; opts->struct_size too small; more than
 * 2^32-1 rows; hash_bits > 63; HMJ_FIRST_WINS; key bytes with chars == NULL; offsets that decrease (checked on the device
 * by the hash kernel: hmj_last_error names the relation and the first offending row, and the ctx stays usable).
 * HMJ_E_UNSUPPORTED wherever the inner ordered u64 join returns it, and for an ordered join with a run of equal hash that
 * holds several distinct matched build keys and more than 1024 rows (or more than 2^22 such adjacent rows in all) --
 * with 64-bit hashes that takes a genuine _Hash_bytes collision.
 * hmj_last_plan / hmj_last_timing describe the inner {hash,row} join.  Its workload memo is keyed apart from plain u64
 * joins (as the kinds' are), so string joins do not change what u64 joins learn.  Like any other call it discards a
 * prepared build side.  Join kinds: hmj_join_kind_str_device below.  NULL keys: hmj_str_join_opts carries no validity
 * bitmap, so this entry joins keys without NULLs; the inner join of nullable keys is the INNER kind of
 * hmj_join_kind_str_device.  Out of scope: the exchange (multi-GPU) path and host-resident string relations.            */
int hmj_join_str_device(hmj_ctx* ctx, const hmj_str_rel* build, const hmj_str_rel* probe, uint32_t flags,
                        hmj_str_join_opts* opts, hmj_str_result* out);

/* The join kinds of hmj_join_kind_u64_device / hmj_join_build_kind_u64_device on string keys.  opts->side and opts->kind
 * select the kind as hmj_exchange_kind_opts does: HMJ_KIND_PROBE_SIDE with HMJ_JOIN_INNER / _SEMI / _ANTI / _PROBE_OUTER,
 * or HMJ_KIND_BUILD_SIDE with HMJ_BUILD_SEMI / _ANTI / _OUTER / HMJ_FULL_OUTER.  Every kind means what it means for the
 * u64 entries, with the string join's match rule (keys equal byte for byte) and its row contents (hash with hash_bits
 * applied, row indices, payloads):
 *   probe SEMI / ANTI            columns hash, s_row, sval (r_row and rval are NULL); each probe row at most once, and
 *                                SEMI + ANTI partition the probe relation;
 *   BUILD_SEMI / BUILD_ANTI      columns hash, r_row, rval (s_row and sval are NULL);
 *   PROBE_OUTER / BUILD_OUTER /  the inner string join's rows, + (hash, HMJ_STR_NO_ROW, s_row, probe_fill, sval) per
 *   FULL_OUTER                   unmatched probe row and / or (hash, r_row, HMJ_STR_NO_ROW, rval, build_fill) per
 *                                unmatched build row, as the kind asks.
 * n_matches = result rows; sum_r / sum_s and HMJ_CHECKSUM's tmix(hash, rval, sval) are taken over result rows, a missing
 * value column counting as 0 and fills as written; HMJ_SUM_PROBE is unchanged.  opts->counts: the counters the u64 entry
 * of the kind fills (probe counters for SEMI / ANTI / PROBE_OUTER, build counters for the build kinds, both for
 * FULL_OUTER), zeros elsewhere.  Empty sides as for the u64 kinds (n_build == 0: ANTI returns every probe row).
 * HMJ_ORDERED (implies HMJ_MATERIALIZE): rows ascending by (hash, key bytes as std::string::operator< orders them, r_row,
 * s_row), HMJ_STR_NO_ROW last; (hash, key bytes, row) for the semi / anti kinds.
 * HMJ_KIND_PROBE_SIDE + HMJ_JOIN_INNER is exactly hmj_join_str_device (rows, sums, order; counters 0).
 * How (DESIGN.md "String keys on the device", join kinds): semi / anti never form the cross product.  The {hash,row} rows
 * are joined first-wins, so every row of the side asked about meets ONE row of its hash on the other side; a verify pass
 * marks the rows whose keys are equal (one byte per row) and lists the others, which -- only after a real hash collision
 * -- are joined with every row of their hash and verified again.  The outer kinds run the inner string join's pair join
 * and verification with the same marks.  One sweep per relation emits the rows its mark selects, stably in row order.
 * Ordered results are sorted by hash (a stable u64 sort of (hash, index) rows) and runs of equal hash with several keys
 * by key bytes, as the inner join sorts them.
 * HMJ_E_ARG: NULL ctx / rel / opts / out, opts->struct_size too small, an unknown side or kind, HMJ_FIRST_WINS, and
 * everything hmj_join_str_device rejects (decreasing offsets included; the ctx stays usable).  HMJ_E_UNSUPPORTED wherever
 * the ordered string join returns it.  hmj_last_plan / hmj_last_timing describe the last internal u64 join; the kinds'
 * workloads are keyed apart from u64 joins, u64 kind joins and the inner string join.
 * NULL keys (Arrow validity bitmaps, hmj_validity below): opts->build_validity / probe_validity give the key column's
 * bitmap of that side, embedded by value (bits == NULL: no NULL on that side; a bitmap on one side only is valid; a call
 * whose two bits are NULL launches exactly the kernels of a call that cannot pass one).  The fields are read and written
 * only when struct_size covers them: a caller built against the header without them -- struct_size up to the offset of
 * build_validity -- gets that header's behaviour bit for bit, whatever bytes lie behind.  hmj_str_join_opts keeps its
 * layout and carries no bitmap: the inner join of nullable string keys is this entry with HMJ_KIND_PROBE_SIDE +
 * HMJ_JOIN_INNER (the same rows, sums, order, n_hash_pairs and n_collisions over the rows that have a key).  SQL's
 * three-valued equality: a NULL-key row matches nothing -- no row of the other side and no other NULL-key row --, so it
 * has no partner, and every kind follows with NOT EXISTS semantics (not NOT IN):
 *   kind          NULL-key probe row                                      NULL-key build row
 *   INNER         not in the result                                       not in the result
 *   probe SEMI    not emitted                                             -
 *   probe ANTI    emitted                                                 -
 *   PROBE_OUTER   unmatched: (0, NO_ROW, s_row, probe_fill, sval)         not in the result
 *   BUILD_SEMI    -                                                       not emitted
 *   BUILD_ANTI    -                                                       emitted
 *   BUILD_OUTER   not in the result                                       unmatched: (0, r_row, NO_ROW, rval, build_fill)
 *   FULL_OUTER    emitted as unmatched                                    emitted as unmatched
 * hash of a NULL-key row is 0 wherever such a row is emitted; the sums and HMJ_CHECKSUM use that 0.  A valid empty string
 * is a key like any other: it matches other valid empty strings and no NULL slot, even one of length zero.  The bytes and
 * the length under a NULL slot are undefined and nothing in the result depends on them -- but the offsets of a NULL slot
 * must still be non-decreasing (Arrow requires it, and the hash kernel stages a wave's whole byte span): a decrease
 * anywhere stays HMJ_E_ARG naming the row, and the ctx stays usable.  chars == NULL stays legal when every slot, valid or
 * NULL, has length 0.  counts: n_*_unmatched includes the NULL-key rows of that side, so SEMI + ANTI still partition the
 * relation; n_build_null / n_probe_null are filled by every kind and are 0 without bitmaps.  n_hash_pairs /
 * n_collisions: NULL-key rows are never paired and count in neither.  HMJ_SUM_PROBE sums every probe row's payload,
 * NULL-key rows included.
 * HMJ_ORDERED: NULL-key rows come after every non-NULL row, among themselves ascending by (r_row, s_row) with
 * HMJ_STR_NO_ROW last -- in a FULL_OUTER result the build side's NULL-key rows by r_row, then the probe side's by s_row --;
 * non-NULL rows keep the order above exactly.  NULL-key rows never enter the hash sort or the collision-run sort (the
 * sweeps emit them into a tail segment of their own), so the 1024-row and 2^22 limits count non-NULL rows only.
 * A side whose rows are all NULL-key behaves as an empty side for matching; its rows are still emitted by the kinds that
 * emit unmatched rows of that side.  HMJ_E_ARG also: bit_offset + n overflows 64 bits.
 * How: a pass over the bitmap alone counts the valid rows per 256-row workgroup (valid_count_kernel), one scan places
 * the workgroups, and str_hash_valid_kernel -- str_hash_kernel with the wave's LDS staging and its unstaged path -- writes
 * the {hash, row} rows of the valid rows only, compacted stably in row order (the u64 joins take those), and for the kinds
 * a dense row-indexed array with {0, HMJ_STR_NO_ROW} for a NULL-key row, which the sweeps walk.  Row indices in the result
 * stay the caller's.
 * NULL-equals-NULL matching (HMJ_NULL_EQUAL, IS NOT DISTINCT FROM) is not taken here: the flag is HMJ_E_ARG, and the message
 * points to hmj_join_mixed_device, which honours it and takes a single string column -- nobody gets SQL semantics silently.
 * Out of scope for NULL keys: validity of the payload column, 32-bit-offset Arrow `string` columns, the exchange path,
 * bitmaps on hmj_join_str_device itself (use the INNER kind).                                                           */
#define HMJ_STR_NO_ROW UINT64_MAX /* r_row / s_row of an outer join's unmatched row: there is no partner             */
typedef struct {
  const void* bits;     /* device: Arrow validity bitmap, least-significant bit first: row i is valid iff
                           (bits[(bit_offset + i) >> 3] >> ((bit_offset + i) & 7)) & 1.  NULL: no NULL in this column.
                           Byte-aligned only; never written                                                  */
  uint64_t bit_offset;  /* Arrow slice offset, any value with bit_offset + n not overflowing                */
} hmj_validity;
typedef struct {
  uint32_t struct_size;   /* in: sizeof(hmj_str_kind_opts) of the caller's header                                       */
  uint32_t side;          /* in: HMJ_KIND_PROBE_SIDE / HMJ_KIND_BUILD_SIDE                                             */
  uint32_t kind;          /* in: a kind of that side                                                                   */
  uint32_t hash_bits;     /* in: as hmj_str_join_opts                                                                  */
  uint64_t probe_fill;    /* in: rval of an unmatched probe row (PROBE_OUTER, FULL_OUTER)                              */
  uint64_t build_fill;    /* in: sval of an unmatched build row (BUILD_OUTER, FULL_OUTER)                              */
  hmj_kind_counts counts; /* out: the counters the u64 entry of the kind fills, zeros elsewhere                        */
  uint64_t n_hash_pairs;  /* out: pairs of equal hash whose keys were compared                                         */
  uint64_t n_collisions;  /* out: of those, pairs whose keys differ                                                    */
  float ms_hash, ms_join, ms_verify, ms_emit, ms_order; /* out, with hmj_set_profiling(ctx, 1): HIP-event phase times  */
  /* NULL keys (above).  Read / written only when struct_size covers them; a shorter struct is a call without bitmaps */
  hmj_validity build_validity;   /* in: the build key column's bitmap; bits == NULL: no NULL on this side */
  hmj_validity probe_validity;   /* in: likewise                                                          */
  uint64_t n_build_null, n_probe_null; /* out: NULL-key rows per side (0 without bitmaps); every kind, INNER included */
} hmj_str_kind_opts;
int hmj_join_kind_str_device(hmj_ctx* ctx, const hmj_str_rel* build, const hmj_str_rel* probe, uint32_t flags,
                             hmj_str_kind_opts* opts, hmj_str_result* out);

/* ---- multi-column fixed-width keys on the device --------------------------------------------------- */
/* The inner equi-join of two relations whose key is a tuple of k fixed-width columns (ON a.x = b.x AND a.y = b.y ...),
 * held on the device as the caller holds them: struct of arrays, one device pointer per column, plus an optional payload
 * column.  Nothing in the reference corresponds: its operator is a template over ONE Key with std::hash<Key>
 * (hashjoin.h:33-56), so a caller of it would pack the tuple into a Key type of its own.  Key construction, the join,
 * tuple verification, payload gather and ordering all run on the GPU; no pass on the host touches keys or rows.         */
#define HMJ_MAX_KEY_COLS 8
typedef struct {
  const void* data;         /* device: n contiguous values of `width` bytes, aligned to `width`                        */
  uint32_t width;           /* 1, 2, 4 or 8                                                                             */
  uint32_t reserved;        /* 0                                                                                        */
} hmj_key_col;
typedef struct {
  const hmj_key_col* cols;  /* HOST array of n_cols entries (read during the call only)                                 */
  uint32_t n_cols;          /* 1 .. HMJ_MAX_KEY_COLS                                                                    */
  uint32_t reserved;        /* 0                                                                                        */
  const uint64_t* vals;     /* device: n payloads; NULL = the payload of row i is i                                     */
  uint64_t n;               /* rows, <= 2^32 - 1                                                                        */
} hmj_cols_rel;
#define HMJ_COLS_PACKED 1u
#define HMJ_COLS_HASHED 2u
typedef struct {
  uint32_t struct_size;     /* in: sizeof of the caller's header (size-versioned like hmj_str_join_opts)               */
  uint32_t hash_bits;       /* in: hashed form only; 0 = 64, 1..63 = h >> (64 - hash_bits): fewer bits make collisions  */
                            /* between different tuples common -- exists so callers and tests can exercise them        */
  uint32_t force_hashed;    /* in: != 0: take the hashed form even when the key fits 8 bytes                            */
  uint32_t form;            /* out: HMJ_COLS_PACKED / HMJ_COLS_HASHED (0 when a side was empty)                         */
  uint64_t n_key_pairs;     /* out: pairs of equal 64-bit join key the {key64,row} join produced                       */
  uint64_t n_collisions;    /* out: of those, pairs whose tuples differ (dropped; always 0 in the packed form)          */
  float ms_key, ms_join, ms_verify, ms_order; /* out, with hmj_set_profiling(ctx, 1): HIP-event phase times             */
} hmj_cols_join_opts;
typedef struct {
  uint64_t n_matches, sum_r, sum_s, xor_fold, mix_sum, sum_probe_all; /* as hmj_str_result; tmix over (key64, rval, sval) */
  const uint64_t *key64, *r_row, *s_row, *rval, *sval; /* HMJ_MATERIALIZE: device columns owned by the ctx, valid  */
                                                       /* until the next call on it / hmj_release_result            */
} hmj_cols_result;
/* Match rule: a result row is a pair (build row, probe row) whose k columns are all equal bit for bit.  Signed integers
 * and floats are compared as their bytes: -0.0 != 0.0, and equal NaN patterns match.  Duplicate tuples on either side
 * give the cross product.  Both relations must have the same n_cols and the same width per column.
 * Row contents: r_row / s_row are row indices into the caller's relations (gather maps; the key columns themselves are
 * not copied out); rval = build->vals[r_row], sval = probe->vals[s_row] (the row index itself where vals is NULL); key64
 * is the 64-bit join key below.
 * The 64-bit join key, with v_c = column c's value zero-extended to 64 bits and T = the sum of the widths:
 *   packed (T <= 8 and not force_hashed)   key64 = v_0 || v_1 || ... || v_{k-1}: column 0 in the most significant
 *                                          position of the T low bytes, the upper 8 - T bytes zero -- i.e.
 *                                          key64 = 0; for c in 0..k-1: key64 = (key64 << (8 * width_c)) | v_c.
 *                                          Equal key64 IS equal tuples: no hash, no verification, no collisions.
 *   hashed                                 h = k; for c in 0..k-1: h = mix64(h + v_c + 0x9E3779B97F4A7C15) (wrapping
 *                                          64-bit sums), with mix64(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9;
 *                                          x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31.  Then
 *                                          key64 = hash_bits ? h >> (64 - hash_bits) : h.
 * Flags: HMJ_MATERIALIZE, HMJ_ORDERED, HMJ_CHECKSUM and HMJ_SUM_PROBE mean what they mean for hmj_join_str_device;
 * HMJ_FIRST_WINS is HMJ_E_ARG.  Without HMJ_MATERIALIZE only the counters and sums are filled; the hashed form still
 * verifies, so every count is exact.
 * HMJ_ORDERED (implies HMJ_MATERIALIZE): rows ascending by (key64, the tuple compared column by column as UNSIGNED
 * integers, r_row, s_row).  In the packed form that is plainly ascending tuple order.  In the hashed form rows of one
 * tuple are contiguous and the order is reproducible from the definition above.
 * How: every row becomes a {key64, row} row (cols_key_kernel: one lane per row, coalesced loads per column, one 16-byte
 * store), the two row sets are joined by the u64 join (HMJ_MATERIALIZE, + HMJ_ORDERED).  Packed: the join's columns are
 * the result's key64 / r_row / s_row; one kernel gathers the payloads and takes the sums.  Hashed: every pair of equal
 * key64 has its tuples compared column by column and its payloads gathered (verify_kernel; survivors compacted
 * stably), and -- ordered only -- runs of equal key64 whose build tuples differ are sorted by tuple, each inside one
 * workgroup.
 * Every tuple is a legal key, the packed tuple of 8 bytes 0xFF (key64 == 2^64 - 1) included: the inner join's global
 * table, whose empty slots hold that value, gives way to the partitioned path for such a build side.
 * n == 0 on either side: an empty result and HMJ_OK (sum_probe_all is still filled when asked).
 * HMJ_E_ARG (hmj_last_error names what was wrong): NULL ctx / rel / opts / out; opts->struct_size too small; n_cols
 * outside 1..HMJ_MAX_KEY_COLS; a NULL cols array; a width other than 1, 2, 4 or 8; a NULL or misaligned data with n > 0;
 * non-zero reserved; different n_cols or widths on the two sides; more than 2^32-1 rows; hash_bits > 63; HMJ_FIRST_WINS.
 * HMJ_E_UNSUPPORTED wherever the inner ordered u64 join returns it, and in the hashed form for an ordered join with a run
 * of equal key64 that holds several distinct matched build tuples and more than 1024 rows (or more than 2^22 such
 * adjacent rows in all) -- with 64 hash bits that takes a genuine collision of the hash above.  The ctx stays usable.
 * hmj_last_plan / hmj_last_timing describe the inner {key64,row} join.  Its workload memo is keyed apart from every
 * other entry's, so multi-column joins do not change what u64 or string joins learn.  Like any other call it discards a
 * prepared build side.  Join kinds: hmj_join_kind_cols_device below.  Out of scope: the exchange (multi-GPU) path,
 * host-resident columns, signed / collated ordering.  The key columns (and any other fixed-width column of either
 * relation) come back through the maps: hmj_take_cols_device below, with r_row / s_row as its row_map.
 * NULL keys (Arrow validity bitmaps, hmj_validity above, in the string section): hmj_cols_join_opts keeps its layout and carries none, so this
 * entry joins columns without NULLs.  The inner join of nullable key columns is hmj_join_kind_cols_device below with
 * HMJ_KIND_PROBE_SIDE + HMJ_JOIN_INNER, whose opts carry one hmj_validity per key column and side: the same rows, sums,
 * order, n_key_pairs and n_collisions over the rows that have a key.                                                     */
int hmj_join_cols_device(hmj_ctx* ctx, const hmj_cols_rel* build, const hmj_cols_rel* probe, uint32_t flags,
                         hmj_cols_join_opts* opts, hmj_cols_result* out);

/* The join kinds of hmj_join_kind_u64_device / hmj_join_build_kind_u64_device on multi-column keys.  opts->side and
 * opts->kind select the kind as hmj_str_kind_opts does: HMJ_KIND_PROBE_SIDE with HMJ_JOIN_INNER / _SEMI / _ANTI /
 * _PROBE_OUTER, or HMJ_KIND_BUILD_SIDE with HMJ_BUILD_SEMI / _ANTI / _OUTER / HMJ_FULL_OUTER.  Every kind means what it
 * means for the u64 entries, with the multi-column join's match rule (all k columns equal bit for bit), its key64
 * (packed or hashed, hash_bits applied) and its row contents (row indices, payloads; vals == NULL: the payload of row i
 * is i, for emitted unmatched rows too):
 *   probe SEMI / ANTI            columns key64, s_row, sval (r_row and rval are NULL); each probe row at most once, and
 *                                SEMI + ANTI partition the probe relation;
 *   BUILD_SEMI / BUILD_ANTI      columns key64, r_row, rval (s_row and sval are NULL);
 *   PROBE_OUTER / BUILD_OUTER /  the inner multi-column join's rows, + (key64, HMJ_COLS_NO_ROW, s_row, probe_fill, sval)
 *   FULL_OUTER                   per unmatched probe row and / or (key64, r_row, HMJ_COLS_NO_ROW, rval, build_fill) per
 *                                unmatched build row, as the kind asks.  key64 of an unmatched row is its own tuple's.
 * n_matches = result rows; sum_r / sum_s and HMJ_CHECKSUM's tmix(key64, rval, sval) are taken over result rows, a missing
 * value column counting as 0 and fills as written; HMJ_SUM_PROBE is unchanged.  opts->counts: the counters the u64 entry
 * of the kind fills (probe counters for SEMI / ANTI / PROBE_OUTER, build counters for the build kinds, both for
 * FULL_OUTER), zeros elsewhere.  opts->form is always filled, empty sides included.
 * Empty sides as for the u64 kinds: n_build == 0: ANTI, PROBE_OUTER and FULL_OUTER return every probe row; n_probe == 0:
 * BUILD_ANTI, BUILD_OUTER and FULL_OUTER return every build row (key64 filled); both empty: an empty result and HMJ_OK.
 * HMJ_ORDERED (implies HMJ_MATERIALIZE): rows ascending by (key64, the tuple compared column by column as UNSIGNED
 * integers, r_row, s_row), HMJ_COLS_NO_ROW last; (key64, tuple, row) for the semi / anti kinds.  In the packed form that
 * is plainly ascending tuple order.
 * HMJ_KIND_PROBE_SIDE + HMJ_JOIN_INNER is exactly hmj_join_cols_device (rows, sums, order, n_key_pairs, n_collisions;
 * counters 0).
 * How (DESIGN.md "Multi-column keys on the device", join kinds): semi / anti never form the cross product.  The
 * {key64,row} rows are joined first-wins, so every row of the side asked about meets ONE row of its key64 on the other
 * side; a verify pass marks the rows whose tuples are equal (one byte per row; packed: every pair, without loading a
 * column) and lists the others, which -- only after a collision of the hash -- are joined with every row of their key64
 * and verified again.  The outer kinds run the inner join's pair join with the same marks (hashed: set by the verification;
 * packed: by the payload gather).  One sweep per relation emits the rows its mark selects, stably in row order.  Ordered
 * results are sorted by key64 (a stable u64 sort of (key64, index) rows) and -- hashed only -- runs of equal key64 with
 * several tuples by tuple, as the inner join sorts them.
 * HMJ_E_ARG: NULL ctx / rel / opts / out, opts->struct_size smaller than through build_fill, an unknown side or a kind
 * not of that side, HMJ_FIRST_WINS, and everything hmj_join_cols_device rejects.  HMJ_E_UNSUPPORTED wherever the ordered
 * inner multi-column join returns it (the same 1024-row and 2^22 limits, over result rows).  The ctx stays usable.
 * hmj_last_plan / hmj_last_timing describe the last internal u64 join; the kinds' workloads are keyed apart from every
 * other entry's.  Like any other call it discards a prepared build side.  Out of scope: as hmj_join_cols_device; the
 * columns of an outer kind's rows, NULL where HMJ_COLS_NO_ROW stands, come from hmj_take_cols_device below.
 * NULL keys (Arrow validity bitmaps): opts->build_validity / probe_validity give one hmj_validity per key column of that
 * side (a NULL array, entries with bits == NULL and bitmaps on one side only are all valid; a call without any bitmap
 * launches exactly the kernels of a call that cannot pass one).  The fields are read and written only when struct_size
 * covers them: a caller built against the header without them gets that header's behaviour bit for bit.  A row is a
 * NULL-key row when at least one of its key columns is NULL in that row.  SQL's three-valued equality: a NULL-key row
 * matches nothing -- no row of the other side and no other NULL-key row --, so it has no partner, and every kind follows
 * with NOT EXISTS semantics (not NOT IN):
 *   kind          NULL-key probe row                                      NULL-key build row
 *   INNER         not in the result                                       not in the result
 *   probe SEMI    not emitted                                             -
 *   probe ANTI    emitted                                                 -
 *   PROBE_OUTER   unmatched: (0, NO_ROW, s_row, probe_fill, sval)         not in the result
 *   BUILD_SEMI    -                                                       not emitted
 *   BUILD_ANTI    -                                                       emitted
 *   BUILD_OUTER   not in the result                                       unmatched: (0, r_row, NO_ROW, rval, build_fill)
 *   FULL_OUTER    emitted as unmatched                                    emitted as unmatched
 * key64 of a NULL-key row is 0 wherever such a row is emitted; the sums and HMJ_CHECKSUM use that 0.  The bytes under a
 * NULL slot are undefined and nothing in the result depends on them.  counts: n_*_unmatched includes the NULL-key rows of
 * that side, so SEMI + ANTI still partition the relation; n_build_null / n_probe_null are filled by every kind and are 0
 * without bitmaps.  n_key_pairs / n_collisions: NULL-key rows are never paired and count in neither.  HMJ_SUM_PROBE sums
 * every probe row's payload, NULL-key rows included.
 * HMJ_ORDERED: NULL-key rows come after every non-NULL row, among themselves ascending by (r_row, s_row) with
 * HMJ_COLS_NO_ROW last -- in a FULL_OUTER result the build side's NULL-key rows by r_row, then the probe side's by s_row --;
 * non-NULL rows keep the order above exactly.  NULL-key rows never enter the sort or the collision sort (the sweeps emit
 * them into a tail segment of their own), so the 1024-row and 2^22 limits count non-NULL rows only.
 * A side whose rows are all NULL-key behaves as an empty side for matching; its rows are still emitted by the kinds that
 * emit unmatched rows of that side.  opts->form is filled as always.  HMJ_E_ARG also: bit_offset + n overflows 64 bits.
 * How: a pass over the bitmaps alone counts the valid rows per workgroup (valid_count_kernel), one scan places the
 * workgroups, and cols_key_valid_kernel writes the {key64,row} rows of the valid rows only, compacted stably in row order;
 * the u64 joins take those.  Row indices in the result stay the caller's.
 * NULL-equals-NULL matching (flags | HMJ_NULL_EQUAL; IS NOT DISTINCT FROM, cuDF's null_equality::EQUAL, pandas' merge,
 * Spark's <=>): the NULL-key table above is replaced by one rule.
 *   Match rule: two rows match when, in every key column, both slots are NULL, or both are valid and equal (bit for bit,
 *   as without the flag).  A NULL slot equals no value: (NULL, 5) does not equal (0, 5), and (NULL, x) does not equal
 *   (x, NULL).  The bytes under a NULL slot stay undefined and nothing depends on them.
 *   key64: 1. h = k.  2. for c in 0..k-1: h = mix64(h + v_c + 0x9E3779B97F4A7C15), with v_c = 0 for a NULL slot and the
 *   hashed form's v_c otherwise.  3. m = the sum of 2^c over the row's NULL columns; if m != 0: h = mix64(h + m +
 *   0x9E3779B97F4A7C15).  4. key64 = hash_bits ? h >> (64 - hash_bits) : h.  A row without NULLs has exactly the hashed
 *   form's key64.
 *   Form: with the flag and at least one bitmap actually passed on either side (an entry with bits != NULL), the call takes
 *   the hashed form, opts->form says so and force_hashed changes nothing.  With the flag and no bitmap the call IS the call
 *   without the flag: the packed form stays available and exactly the same kernels are launched.
 *   Kinds: a row with NULL slots is an ordinary row for all eight (side, kind) pairs -- matched, marked, emitted and counted
 *   in n_*_matched / n_*_unmatched like any other; emitted unmatched, its key64 is its own key64, not 0.  A relation whose
 *   rows are all NULL is not an empty side: its rows match the other side's rows with the same NULL columns.
 *   n_build_null / n_probe_null still report the rows with at least one NULL key column (informational; every kind).
 *   n_key_pairs / n_collisions count these rows' pairs as they count any others.
 *   HMJ_ORDERED: rows ascending by (key64, the tuple column by column, r_row, s_row), HMJ_COLS_NO_ROW last; in each column
 *   a NULL slot sorts after every valid value (NULLS LAST) and two NULL slots tie.  There is no tail segment, and the
 *   1024-row and 2^22 limits count all rows.
 *   How: cols_key_ne_kernel, one lane per row, reads a column's 64 validity bits per wave as one or two aligned 8-byte
 *   words, substitutes v_c = 0, mixes m in and writes one dense {key64, row} row per row -- no count pass, no scan, no
 *   compaction; the rest is the hashed form's sequence on a key policy that compares validity before values.
 *   Without the flag every call behaves and launches exactly as before.  hmj_join_cols_device (no bitmaps) ignores it.
 * Out of scope for NULL keys: validity of the payload column, the exchange path, bitmaps in hmj_cols_join_opts (use the
 * INNER kind here).  String keys' validity is not part of this entry: hmj_join_kind_str_device takes it under SQL
 * semantics, hmj_join_mixed_device under either.                                                                        */
#define HMJ_COLS_NO_ROW UINT64_MAX /* r_row / s_row of an outer join's unmatched row: there is no partner            */
typedef struct {
  uint32_t struct_size;   /* in: sizeof(hmj_cols_kind_opts) of the caller's header                                     */
  uint32_t side;          /* in: HMJ_KIND_PROBE_SIDE / HMJ_KIND_BUILD_SIDE                                             */
  uint32_t kind;          /* in: a kind of that side                                                                   */
  uint32_t hash_bits;     /* in: as hmj_cols_join_opts                                                                 */
  uint32_t force_hashed;  /* in: as hmj_cols_join_opts                                                                 */
  uint32_t form;          /* out: HMJ_COLS_PACKED / HMJ_COLS_HASHED -- always filled, empty sides included             */
  uint64_t probe_fill;    /* in: rval of an unmatched probe row (PROBE_OUTER, FULL_OUTER)                              */
  uint64_t build_fill;    /* in: sval of an unmatched build row (BUILD_OUTER, FULL_OUTER)                              */
  hmj_kind_counts counts; /* out: the counters the u64 entry of the kind fills, zeros elsewhere                        */
  uint64_t n_key_pairs;   /* out: pairs of equal key64 that were compared (packed: formed)                             */
  uint64_t n_collisions;  /* out: of those, pairs whose tuples differ (packed: 0)                                       */
  float ms_key, ms_join, ms_verify, ms_emit, ms_order; /* out, with hmj_set_profiling(ctx, 1): HIP-event phase times   */
  /* NULL keys (above).  Read / written only when struct_size covers them; a shorter struct is a call without bitmaps */
  const hmj_validity* build_validity; /* in: HOST array of n_cols entries (read during the call only), or NULL */
  const hmj_validity* probe_validity; /* in: likewise                                                          */
  uint64_t n_build_null, n_probe_null; /* out: NULL-key rows per side (0 without bitmaps); every kind, INNER included */
} hmj_cols_kind_opts;
int hmj_join_kind_cols_device(hmj_ctx* ctx, const hmj_cols_rel* build, const hmj_cols_rel* probe, uint32_t flags,
                              hmj_cols_kind_opts* opts, hmj_cols_result* out);

/* ---- mixed keys: string and fixed-width columns in one tuple ----------------------------------------- */
/* The joins of hmj_join_kind_cols_device on a key tuple whose columns are Arrow large_string columns and fixed-width
 * columns in any order (ON a.name = b.name AND a.day = b.day; two string columns; ...).  One entry for all eight (side,
 * kind) pairs, HMJ_KIND_PROBE_SIDE + HMJ_JOIN_INNER included; the result struct is hmj_cols_result.  The key is always
 * hashed: a caller whose columns are all fixed-width should prefer hmj_join_kind_cols_device, whose packed form needs no
 * verification; fixed-only and string-only column sets are still legal here.  Nothing in the reference corresponds (one
 * Key type per operator, hashjoin.h:33-56).
 * Everything the header text of hmj_join_kind_cols_device says holds here word for word -- kinds and their columns, row
 * contents (row indices, payloads; vals == NULL: the payload of row i is i), sums and checksums, counts, empty sides,
 * flags (HMJ_FIRST_WINS is HMJ_E_ARG), the NULL-key table -- with these points changed:
 * Match rule: every column equal.  A fixed column is equal bit for bit; a string column byte for byte -- equal length and
 * equal bytes, NUL and bytes >= 0x80 being ordinary bytes.  Both relations need the same n_cols and, per column, the same
 * type and width.
 * key64: h = k; for c in 0..k-1: h = mix64(h + v_c + 0x9E3779B97F4A7C15) (hmj_join_cols_device's hashed form), with
 *   v_c = the column's value zero-extended to 64 bits                         for a fixed column,
 *   v_c = libstdc++'s _Hash_bytes of the slot's bytes, all 64 bits, seed 0xc70f6907 -- std::hash<std::string>, what
 *         hmj_hash_str_device returns with hash_bits 0 --                      for a string column;
 *   key64 = hash_bits ? h >> (64 - hash_bits) : h.  A string's length is inside _Hash_bytes, so ("ab","c") and ("a","bc")
 *   differ before verification, and they differ after it.
 * HMJ_ORDERED: rows ascending by (key64, the tuple column by column, r_row, s_row), HMJ_COLS_NO_ROW last: fixed columns
 * compare as unsigned integers, string columns as std::string::operator< (unsigned bytes, then length).  NULL-key rows go
 * into the tail exactly as in the column join.
 * NULL keys: the bitmaps are part of the columns (hmj_mixed_col.validity; bits == NULL: no NULL in the column).  A row is
 * a NULL-key row when any key column is NULL in it: the same eight-row table, key64 0, counters and n_build_null /
 * n_probe_null.  A valid empty string is a key.  The bytes and the length under a NULL slot are undefined, but its
 * offsets must still be non-decreasing.  A call without any bitmap launches neither valid_count_kernel nor its scan.
 * HMJ_E_ARG (hmj_last_error names what was wrong): everything hmj_join_kind_cols_device rejects; an unknown type; width
 * != 0 on a string column or offsets != NULL on a fixed one; NULL offsets with n > 0 (or offsets not aligned to 8 bytes);
 * a type or width that differs between the sides (the message names the column); bit_offset + n overflowing 64 bits; key
 * bytes under data == NULL; decreasing offsets.  The last two are found on the device by the key kernel, before anything
 * reads a key byte through them: hmj_last_error names the relation, the lowest-numbered offending column and, for
 * decreasing offsets, that column's first offending row.  The ctx stays usable.
 * HMJ_E_UNSUPPORTED where the column join returns it, with the same 1024-row and 2^22 limits.
 * The result lives until the next call on the ctx / hmj_release_result.  r_row / s_row are valid row maps for
 * hmj_take_cols_device (fixed columns) and hmj_take_str_device (string columns).  hmj_last_plan / hmj_last_timing
 * describe the last internal u64 join; the workloads are keyed apart from every other entry's (workload kinds 20..24), and
 * the entry has a workspace of its own.  Like any other call it discards a prepared build side.
 * How (DESIGN.md "Mixed keys (string and fixed-width columns)"): mix_key_kernel, one lane per row, walks the columns
 * once -- a fixed column is one coalesced load per wave; for a string column the wave stages its 64 keys' byte span in
 * LDS as the string join's hash kernel does -- and writes one {key64, row} row; the rest is the column join's sequence on
 * a key policy that compares fixed columns first, then string lengths, then bytes.
 * NULL-equals-NULL matching (flags | HMJ_NULL_EQUAL): as written for hmj_join_kind_cols_device -- match rule, key64 (v_c =
 * 0 for a NULL slot of either type, then the mask step), kinds, counters, NULLS LAST order without a tail -- with the
 * bitmaps in hmj_mixed_col.validity; a call that passes the flag and no bitmap is the call without the flag.  A NULL
 * string slot does not equal the valid empty string (whose v_c is _Hash_bytes of no bytes, not 0).  The bytes and the
 * length under a NULL slot stay undefined and are neither hashed nor compared, but its offsets must still be
 * non-decreasing; the decreasing-offsets and `data == NULL but keys have bytes` checks behave as without the flag.  A
 * string-only column set is legal, so this is also the NULL-equals-NULL string join (hmj_join_kind_str_device refuses
 * the flag).  mix_key_kernel's NULL-equals-NULL variant reads the validity words per wave and column as the column join's.
 * Out of scope: 32-bit-offset `string` columns, the exchange (multi-GPU) path, host-resident columns, collated or signed
 * ordering, a packed form for mixed keys.                                                                              */
#define HMJ_KEY_FIXED 0u
#define HMJ_KEY_LARGE_STRING 1u
typedef struct {
  uint32_t type;            /* HMJ_KEY_FIXED / HMJ_KEY_LARGE_STRING                                              */
  uint32_t width;           /* FIXED: 1, 2, 4 or 8.  LARGE_STRING: 0                                             */
  const void* data;         /* FIXED: n values aligned to width.  LARGE_STRING: the chars buffer (unaligned is   */
                            /* fine; NULL is legal when every slot, valid or NULL, has length 0)                 */
  const uint64_t* offsets;  /* LARGE_STRING: n + 1 non-decreasing offsets, offsets[0] need not be 0. FIXED: NULL */
  hmj_validity validity;    /* bits == NULL: no NULL in this column                                              */
} hmj_mixed_col;
typedef struct {
  const hmj_mixed_col* cols; /* HOST array of n_cols entries (read during the call only); what they point to: device */
  uint32_t n_cols, reserved; /* 1 .. HMJ_MAX_KEY_COLS; 0                                                              */
  const uint64_t* vals;      /* device: n payloads; NULL = the payload of row i is i                                  */
  uint64_t n;                /* rows, <= 2^32 - 1                                                                     */
} hmj_mixed_rel;
typedef struct {
  uint32_t struct_size, side, kind, hash_bits; /* in: sizeof of the caller's header (at least through build_fill); as hmj_cols_kind_opts */
  uint64_t probe_fill, build_fill;             /* in: as hmj_cols_kind_opts                                                               */
  hmj_kind_counts counts;                      /* out: as hmj_cols_kind_opts (zeros for INNER)                                            */
  uint64_t n_key_pairs, n_collisions, n_build_null, n_probe_null; /* out: as hmj_cols_kind_opts                                           */
  float ms_key, ms_join, ms_verify, ms_emit, ms_order; /* out, with hmj_set_profiling(ctx, 1) (INNER: ms_emit 0)                          */
} hmj_mixed_opts;
int hmj_join_mixed_device(hmj_ctx* ctx, const hmj_mixed_rel* build, const hmj_mixed_rel* probe, uint32_t flags,
                          hmj_mixed_opts* opts, hmj_cols_result* out);

/* ---- grouping rows by multi-column keys (GROUP BY / DISTINCT) ------------------------------------------ */
/* The rows of ONE relation of hmj_join_cols_device's shape (k fixed-width key columns, struct of arrays, an optional
 * payload column) are grouped by their key tuple on the device: SELECT DISTINCT a, b; COUNT(*) per foreign key, to size a
 * join's result; GROUP BY a, b with COUNT / SUM / MIN / MAX of one unsigned 64-bit value column.  Nothing in the reference
 * corresponds.  A new entry with structs of its own: no other struct, flag or path bit changes.
 * Grouping rule: two rows are in one group when, in every key column, both slots are NULL, or both are valid and equal bit
 * for bit -- HMJ_NULL_EQUAL's match rule, always on here (SQL's GROUP BY, pandas' dropna=False): the NULLs of a column form
 * one group, (NULL, 5) and (0, 5) are different groups, and so are (NULL, x) and (x, NULL).  The bytes under a NULL slot are
 * undefined and nothing depends on them.  Every row belongs to exactly one group.  A caller who wants pandas' default drops
 * the groups whose first_row is NULL in a key column; a take of the key columns with validity tells which.
 * HMJ_NULL_EQUAL in flags is accepted and ignored (it is implied).
 * key64 and form are exactly hmj_join_kind_cols_device's under HMJ_NULL_EQUAL.  Packed: T <= 8, not force_hashed and no
 * entry of opts->validity with bits != NULL; key64 is the tuple itself.  Otherwise hashed, with the NULL-column mask step
 * (a row without NULLs has the plain hashed key64); hash_bits is applied last.  opts->form is always filled.
 * Outputs.  Without HMJ_MATERIALIZE only n_groups, n_rows, max_count, opts->n_null, opts->n_collisions and opts->form are
 * filled (COUNT(DISTINCT ...)); every column pointer is NULL.  With HMJ_MATERIALIZE key64 and first_row are always filled:
 * first_row is the SMALLEST row index of the group, so the representative is deterministic, and a take of the key columns
 * through first_row (hmj_take_cols_device) is the DISTINCT table.  The HMJ_GROUP_* bits of opts->want add count, sum / min /
 * max and group_of_row; a column not asked for is NULL.  sum / min / max run over rel->vals, or over the row index where
 * vals is NULL; sum wraps mod 2^64, min / max compare unsigned.  group_of_row[i] is the index of row i's group into the
 * group columns.  The result is owned by the ctx and valid until the next call on it or hmj_release_result; the calls
 * that say so keep it: hmj_take_cols_device, hmj_take_str_device, hmj_group_agg_device, hmj_filter_device and
 * hmj_order_by_device.  Like any other call this one discards a prepared build side.
 * Order of groups.  HMJ_ORDERED (implies HMJ_MATERIALIZE): ascending by (key64, the tuple column by column as UNSIGNED
 * integers, NULLS LAST in each column) -- in the packed form plainly ascending tuple order, i.e. GROUP BY ... ORDER BY the
 * keys.  Without it the order is unspecified; all group columns agree with each other and with group_of_row.
 * n == 0: n_groups == 0 and HMJ_OK.
 * HMJ_E_ARG (hmj_last_error names what was wrong): everything hmj_join_cols_device rejects for one relation (NULL ctx / rel
 * / opts / out, n_cols, widths, NULL or misaligned data, non-zero reserved, more than 2^32-1 rows, hash_bits > 63);
 * HMJ_FIRST_WINS, HMJ_CHECKSUM, HMJ_SUM_PROBE; unknown want bits; non-zero opts->reserved; struct_size smaller than through
 * validity; a bit_offset + n that overflows 64 bits.
 * HMJ_E_UNSUPPORTED, the hashed form's limit: a run of equal key64 that holds several distinct tuples and more than 1024
 * rows, or more than 2^22 adjacent sorted rows of equal key64 with different tuples.  Unlike the joins, which meet it in
 * ordered calls only, it applies to every call here: no group can be formed without resolving such a run.  With 64 hash bits
 * that takes a genuine collision of the hash.  The ctx stays usable.
 * How (DESIGN.md "Grouping rows by multi-column keys"): the join's key kernel writes {key64, row} rows, hmj_sort_u64_device
 * sorts them stably (rows of one key64 ascending by row), the hashed form sorts runs of equal key64 with several tuples by
 * (tuple, row) in one workgroup each, group_heads_kernel marks every position whose key differs from its predecessor's
 * (a wave's ballot is 64 head bits; one scan places the workgroups; tuples are compared only in a call whose collision
 * search found a mismatch), group_emit_kernel writes the group columns and the row map, and group_agg_kernel reduces the
 * payloads by a segmented scan inside each wave, finishing a group that crosses the 512 positions a wave walks with one
 * atomic per wave.  Everything runs on the ctx stream in a workspace of the entry's own; the host reads back the
 * mismatch count, n_groups and one counter block.  hmj_last_plan / hmj_last_timing are left as they were.
 * String and mixed keys: hmj_group_mixed_device below.
 * Several value columns per call, signed and float aggregates, NULL values: hmj_group_agg_device below, over this call's
 * grouping.  Out of scope: the exchange path.                                                                          */
#define HMJ_GROUP_COUNT   0x01u  /* out->count                                                                         */
#define HMJ_GROUP_SUM     0x02u  /* out->sum: wrapping u64 sum of the payloads                                          */
#define HMJ_GROUP_MIN     0x04u  /* out->min: unsigned                                                                  */
#define HMJ_GROUP_MAX     0x08u  /* out->max: unsigned                                                                  */
#define HMJ_GROUP_ROW_MAP 0x10u  /* out->group_of_row                                                                   */
typedef struct {
  uint32_t struct_size;          /* in: sizeof of the caller's header (size-versioned like hmj_cols_kind_opts)          */
  uint32_t want;                 /* in: HMJ_GROUP_* bits; any other bit is HMJ_E_ARG                                     */
  uint32_t hash_bits;            /* in: as hmj_cols_join_opts                                                           */
  uint32_t force_hashed;         /* in: as hmj_cols_join_opts                                                           */
  uint32_t form;                 /* out: HMJ_COLS_PACKED / HMJ_COLS_HASHED, always filled                               */
  uint32_t reserved;             /* 0                                                                                   */
  const hmj_validity* validity;  /* in: HOST array of n_cols entries (read during the call only), or NULL               */
  uint64_t n_null;               /* out: rows with at least one NULL key slot                                           */
  uint64_t n_collisions;         /* out: adjacent sorted rows of equal key64 whose tuples differ (packed: 0)            */
  float ms_key, ms_sort, ms_groups, ms_agg; /* out, with hmj_set_profiling(ctx, 1): HIP-event phase times              */
} hmj_group_opts;
typedef struct {
  uint64_t n_groups, n_rows;
  uint64_t max_count;            /* rows of the largest group (0 when n == 0)                                           */
  const uint64_t *key64, *first_row, *count, *sum, *min, *max; /* n_groups each; device, HMJ_MATERIALIZE               */
  const uint64_t* group_of_row;  /* n_rows; device, HMJ_MATERIALIZE + HMJ_GROUP_ROW_MAP                                 */
} hmj_group_result;
int hmj_group_cols_device(hmj_ctx* ctx, const hmj_cols_rel* rel, uint32_t flags, hmj_group_opts* opts,
                          hmj_group_result* out);

/* ---- grouping rows by string and mixed keys ------------------------------------------------------------ */
/* hmj_group_cols_device on ONE relation of hmj_join_mixed_device's shape: any mix of HMJ_KEY_FIXED and
 * HMJ_KEY_LARGE_STRING key columns (strings only and fixed columns only included), validity in the columns, rel->vals the
 * one value column: GROUP BY name; SELECT DISTINCT name, day; COUNT(*) per string foreign key.  hmj_group_opts and
 * hmj_group_result are reused unchanged; no struct, flag or path bit is new.
 * Everything the header text of hmj_group_cols_device says holds here -- outputs, want bits, first_row, aggregates, n == 0,
 * the flags refused, HMJ_NULL_EQUAL accepted and ignored, result lifetime, hmj_last_plan / hmj_last_timing left as they
 * were, a prepared build side discarded -- with these points changed:
 * Grouping rule: in every column both slots NULL, or both valid and equal: a fixed column bit for bit, a string column in
 * length and bytes (NUL and bytes >= 0x80 being ordinary bytes).  A NULL string is not the empty string.  Chars and fixed
 * values under a NULL slot are never read; the offsets under a NULL slot must still be non-decreasing.
 * key64 and form: always hashed -- opts->form is HMJ_COLS_HASHED, opts->force_hashed is ignored.  key64 is
 * hmj_join_mixed_device's under HMJ_NULL_EQUAL: the plain mixed chain for a row without NULL slots, v_c = 0 for a NULL
 * slot and the NULL-column mask step for a row with one, hash_bits last.  For a relation of fixed columns only that is
 * hmj_group_cols_device's hashed key64, and every output equals that entry's with force_hashed.
 * opts->validity must be NULL (the bitmaps are hmj_mixed_col.validity).
 * HMJ_ORDERED: ascending by (key64, the tuple column by column, NULLS LAST in each column): fixed columns as unsigned
 * integers, string columns as std::string::operator< (unsigned bytes, then length).
 * HMJ_E_ARG (hmj_last_error names what was wrong): what hmj_group_cols_device rejects in opts and flags; non-NULL
 * opts->validity; everything hmj_join_mixed_device rejects for one relation (the messages name the "grouped" relation);
 * key bytes under data == NULL; decreasing offsets, the message naming the lowest-numbered offending column and its first
 * offending row in hmj_join_mixed_device's wording.  The last two are found by the key kernel; the host reads its verdict
 * back behind the sort of the {key64, row} rows and before any kernel follows an offset into chars.  The ctx stays usable.
 * HMJ_E_UNSUPPORTED: hmj_group_cols_device's 1024-row and 2^22 limits, in every mode.
 * The result lives in hmj_group_cols_device's workspace: either group call replaces the other's result;
 * hmj_take_cols_device and hmj_take_str_device keep it, and a take of a string key column through first_row is the
 * DISTINCT table.
 * How (DESIGN.md "Grouping rows by string and mixed keys"): mix_key_kernel's dense forms write the rows, and the sequence
 * of hmj_group_cols_device runs on the mixed join's key policies (MixSide; MixNeSide where a column has a bitmap).  One
 * round trip more than the column entry: the key kernel's verdict.
 * Several value columns per call, signed and float aggregates, NULL values: hmj_group_agg_device below, over this call's
 * grouping.  Out of scope: 32-bit-offset `string` columns, the exchange path, a sort-free path for few groups.         */
int hmj_group_mixed_device(hmj_ctx* ctx, const hmj_mixed_rel* rel, uint32_t flags, hmj_group_opts* opts,
                           hmj_group_result* out);

/* ---- aggregating typed value columns over a grouping (SUM / MIN / MAX / MEAN / COUNT) ------------------ */
/* What turns a grouping into a query result: up to HMJ_MAX_AGGS aggregates of typed, NULL-aware value columns are reduced
 * over the groups of the ctx's LIVE GROUPING in one call -- SUM(price), AVG(qty), MIN(ts) over an int32, a float64 and an
 * int64 column.  The counterpart of hmj_take_cols_device for the group entries.  Nothing in the reference corresponds.  A
 * new entry with structs of its own: no other entry, struct, flag or path bit changes.
 * src and dst are HOST arrays of n_aggs entries (read during the call only; dst[a].null_count is written); everything they
 * point to is on the device and caller-owned.  One source column may appear in several entries (SUM and MIN of one column).
 * Binding.  The live grouping is the last successful hmj_group_cols_device or hmj_group_mixed_device call made with
 * HMJ_MATERIALIZE (HMJ_ORDERED implies it).  Output slot g of every aggregate belongs to group g of that call's group
 * columns: the index of key64[g], first_row[g], count[g] and of group_of_row.  n_rows must equal that call's n_rows, and
 * row i of every source column is row i of the grouped relation.  The binding begins when such a call returns HMJ_OK.  It
 * ends at the entry of the next group call on the ctx -- whether that call succeeds or not, count-only calls included --, at
 * hmj_release_result and at hmj_destroy.  No other entry touches the group workspace: joins, sorts, takes and earlier
 * aggregate calls in between keep the binding.  Without a live grouping the call is HMJ_E_ARG ("no live grouping").
 * The call has a workspace of its own and leaves the last result (the group columns included), a prepared build side,
 * hmj_last_plan, hmj_last_timing and the workload memos as they were.  It returns with the work complete on the ctx stream;
 * opts->n_groups is filled.
 * Semantics; every output is a function of the inputs and the grouping alone.
 * Validity: source slot i of aggregate a is NULL where bit bit_offset + i of src[a].validity.bits is 0 (an Arrow bitmap at
 * any bit_offset; bits == NULL: the column has no NULL).  NULL values are skipped, and whatever lies under a NULL slot is
 * never used.  HMJ_AGG_COUNT is the number of valid values of the group -- without a bitmap the group's size --, always a
 * valid uint64; its data may be NULL and its type is ignored beyond being a known one.
 * Empty groups: a group without a valid value gives a NULL output slot for SUM, MIN, MAX and MEAN, its value bytes written
 * as 0.  dst[a].validity != NULL: ceil(n_groups / 64) 64-bit words are written exactly as hmj_take_dst's (group g = bit
 * g & 63 of word g >> 6, padding bits 0).  dst[a].null_count is filled with or without a bitmap.
 * SUM: signed integers are sign-extended and summed in int64, unsigned ones zero-extended and summed in uint64, both
 * wrapping; F32 and F64 are summed in double (an F32 value converts exactly).  The output is int64 / uint64 / double.
 * MIN / MAX: the output has the source type.  Integers compare in their own signedness; floats by IEEE order with
 * -0.0 < +0.0; a NaN loses against any number, and a group whose valid values are all NaN gives the canonical quiet NaN
 * (0x7ff8000000000000, 0x7fc00000).
 * MEAN: double -- the double sum of the values, each converted to double, divided by the valid count (not the wrapped
 * integer sum).
 * Float sums are deterministic: the bits depend on the inputs and on the grouping only -- the same call gives the same bits
 * whatever ran before it.  The order of the additions is fixed by the sorted positions of the group's rows (a segmented
 * scan inside chunks of 64 positions, chunks in ascending order inside the 512 positions a wave walks, then the waves'
 * partials in ascending order in a fixed shape); there is no floating-point atomic and no integer one either.  The sum is
 * NOT the correctly rounded one: |sum - exact| <= gamma_k * sum|x| with gamma_k = k u / (1 - k u), u = 2^-53, k the valid
 * count, as for any order of summation.
 * n_rows == 0 (a live grouping of zero rows): HMJ_OK, n_groups 0, null_count 0, nothing is written on the device.
 * HMJ_E_ARG, found by the host before any launch (hmj_last_error names what was wrong): NULL ctx / src / dst / opts;
 * opts->struct_size smaller than through `reserved`; non-zero reserved; n_aggs outside 1..HMJ_MAX_AGGS; an unknown type or
 * op; NULL data except for HMJ_AGG_COUNT, or data misaligned to the value's width, when n_rows > 0; NULL dst[a].data when
 * there are groups; dst[a].data misaligned to the output's width; dst[a].validity not aligned to 8 bytes; bit_offset + n_rows
 * overflowing 64 bits; no live grouping; n_rows differing from the live grouping's; a destination range (data or bitmap)
 * that overlaps a source column, a source bitmap or another destination of the call (address ranges).  The ctx stays usable
 * after any error.
 * How (DESIGN.md "Aggregating typed columns over a grouping"): per launch chunk of up to 4 aggregates three kernels run
 * over the grouping's sorted {key64,row} rows, head ballots and group starts.  agg_walk_kernel: group_agg_kernel's walk -- a
 * wave covers 8 chunks of 64 sorted positions, the row index and the ballot word are loaded once for all aggregates, every
 * gather of a position (values and validity bytes) is issued before the segmented __shfl_up scan; an aggregate that names
 * the source column or bitmap of the one in front of it (SUM(x), MIN(x), MAX(x)) reuses its load -- with a 64-bit
 * accumulator and a valid count per aggregate (integer sums as u64, float sums and means as double, MIN / MAX on an
 * order-preserving u64 key); a group inside the wave's range is stored by its last lane, the at most two groups open at the
 * range's ends go to the wave's left and right partial slots.  agg_combine_kernel: one wave per group that reaches a wave
 * boundary reduces its partials, strided over the lanes in ascending wave order, then a fixed shuffle tree.
 * agg_finish_kernel: one lane per group converts the accumulator (MEAN divides, MIN / MAX unmap, NULL slots become 0),
 * stores the value, stores a wave's ballot as one bitmap word and counts NULLs by popcount, one atomic per workgroup; that
 * counter block is the call's one read-back.
 * Out of scope: variance / stddev, string MIN / MAX, COUNT(DISTINCT value), decimal128, the exchange path, host-resident
 * columns.                                                                                                              */
#define HMJ_AGG_COUNT 0u  /* valid (non-NULL) values of the group -> uint64, never NULL                                 */
#define HMJ_AGG_SUM   1u  /* -> int64 (signed types), uint64 (unsigned types), double (F32 / F64)                        */
#define HMJ_AGG_MIN   2u  /* -> the source type                                                                         */
#define HMJ_AGG_MAX   3u  /* -> the source type                                                                         */
#define HMJ_AGG_MEAN  4u  /* -> double                                                                                  */
#define HMJ_TYPE_I8  0u
#define HMJ_TYPE_I16 1u
#define HMJ_TYPE_I32 2u
#define HMJ_TYPE_I64 3u
#define HMJ_TYPE_U8  4u
#define HMJ_TYPE_U16 5u
#define HMJ_TYPE_U32 6u
#define HMJ_TYPE_U64 7u
#define HMJ_TYPE_F32 8u
#define HMJ_TYPE_F64 9u
#define HMJ_MAX_AGGS 64
typedef struct {
  const void* data;       /* device: n_rows values of `type`, aligned to their width; may be NULL for HMJ_AGG_COUNT */
  uint32_t type;          /* HMJ_TYPE_*                                                                          */
  uint32_t op;            /* HMJ_AGG_*                                                                           */
  hmj_validity validity;  /* source bitmap, any bit_offset; bits == NULL: the column has no NULL                  */
} hmj_agg_src;
typedef struct {
  void* data;             /* device, caller-owned: n_groups values of the aggregate's output type, aligned to it  */
  uint64_t* validity;     /* device, caller-owned, or NULL: ceil(n_groups / 64) 64-bit words; Arrow bitmap at bit
                             offset 0, group g = bit g, padding bits written as 0                                */
  uint64_t null_count;    /* out: NULL slots of this output column (filled with or without bitmap)               */
} hmj_agg_dst;
typedef struct {
  uint32_t struct_size;   /* size-versioned like the other opts                                                  */
  uint32_t reserved;
  uint64_t n_groups;      /* out: the live grouping's groups = the slots written per aggregate                   */
  float ms_agg;           /* out, with hmj_set_profiling                                                         */
} hmj_group_agg_opts;
int hmj_group_agg_device(hmj_ctx* ctx, const hmj_agg_src* src, uint32_t n_aggs, uint64_t n_rows, hmj_agg_dst* dst,
                         hmj_group_agg_opts* opts);

/* ---- ordering rows by typed, string and mixed keys (ORDER BY) -------------------------------------------- */
/* A stable multi-column ORDER BY: up to HMJ_MAX_ORDER_COLS key columns -- fixed-width columns of the ten HMJ_TYPE_* value
 * types and Arrow large_string columns (64-bit offsets), each with its own direction, NULL placement and optional validity
 * bitmap -- give a row map: row_map_out[j] is the index of the row at sorted position j.  The map is what
 * hmj_take_cols_device and hmj_take_str_device consume, so `GROUP BY name ORDER BY sum(price) DESC, name` stays on the
 * device: group -> aggregate -> order by the aggregate column and the taken key column -> take.  Every other "ordered" mode
 * of the library sorts by (key64, tuple as unsigned integers) -- hash order for hashed and string keys; this entry is the
 * one that orders by value.  Nothing in the reference corresponds beyond its u64 sort (radix_sort.h), which the call uses.
 * A new entry with structs of its own: no other entry, struct, flag or path bit changes.
 * cols is a HOST array of n_cols entries (read during the call only); everything it points to is on the device.
 * row_map_out is caller-owned device memory of n uint64, aligned to 8.  n is at most 2^32 - 1.
 * Order.  Rows compare column by column in the order of cols.  Within a column: two NULL slots (validity bit 0) are equal; a
 * NULL slot sorts after every valid value, and before every valid value under HMJ_ORDER_NULLS_FIRST -- absolutely:
 * HMJ_ORDER_DESC reverses the order of VALID values only.  Integers compare in their own signedness.  Floats compare in IEEE
 * order with -0.0 < +0.0 (hmj_group_agg_device's rule); every NaN, whatever its sign and payload, is ONE value above +inf
 * (so first among the valid values under HMJ_ORDER_DESC).  Strings compare as std::string::operator< does: unsigned bytes,
 * then length; NUL and bytes >= 0x80 are ordinary bytes; a NULL string is not the empty string.  Rows equal in every column
 * keep ascending row index: the sort is stable and the map is unique.  What lies under a NULL slot is never read (value
 * bytes, string bytes); a string column's offsets are read for every row and must be non-decreasing under NULL slots too.
 * Context.  The call runs on the ctx stream in a workspace of its own and returns with the map complete.  It calls
 * hmj_sort_u64_device and shares its effects: a prepared build side is discarded, and the lifetime of the last JOIN result
 * ends (take a join's columns before ordering them).  hmj_last_plan / hmj_last_timing keep describing the last join.  The
 * group result and the live grouping of hmj_group_agg_device are kept.  What the sorts learn is kept under a workload
 * signature of its own (kind 25).
 * opts (out): n_distinct -- distinct key tuples; n_tied_rows -- rows whose whole key equals another row's; n_rounds -- sort
 * rounds run (0 when n <= 1); with hmj_set_profiling ms_key (the key kernel), ms_sort (the first sort), ms_map (heads,
 * active rows and the map behind the first sort), ms_refine (every later round).
 * n == 0: HMJ_OK, nothing is written and no argument that is only checked with n > 0 is looked at.  n == 1: the map is
 * {0}; the columns are not read (no offsets check) and no sort runs, so a prepared build side is still discarded but the
 * last join result stays as it was.
 * HMJ_E_ARG, found by the host before any launch (hmj_last_error names what was wrong): NULL ctx / cols / opts; NULL or
 * misaligned row_map_out with n > 0; n_cols outside 1..HMJ_MAX_ORDER_COLS; an unknown type or flag bit; non-zero reserved /
 * reserved2; opts->struct_size smaller than through `reserved2`; NULL or misaligned data of a fixed column with n > 0;
 * offsets set on a fixed column, or NULL / not aligned to 8 on a string column; bit_offset + n overflowing 64 bits; more
 * than 2^32 - 1 rows; row_map_out overlapping a column's values, offsets or bitmap (address ranges; the extent of a string
 * column's chars is known on the device only and is not checked).  Found on the device by the key kernel, before anything
 * follows an offset into chars, in the mixed-key join's wording (lowest-numbered offending column, first offending row):
 * decreasing offsets, and key bytes of a VALID slot under data == NULL (a NULL slot holds no key bytes, whatever its
 * offsets span).  The ctx stays usable after any error.
 * How (DESIGN.md "Ordering rows (ORDER BY)").  Every row has an order-preserving byte stream whose memcmp order is the
 * requested order: per column a marker byte when the column has a bitmap (0 / 1, the NULL side as flagged), then a fixed
 * value big-endian (sign bit flipped; floats: negative complemented, else sign bit set, NaN all ones; zeros under a NULL
 * slot) or a string as 8-byte blocks of 7 data bytes (zero padded) and a control byte (0xFF: the string continues, else
 * the block's data bytes 0..7; max(1, ceil(len / 7)) blocks; nothing under a NULL slot); HMJ_ORDER_DESC complements the
 * value bytes.  The stream is prefix-free.  order_key_kernel writes {first 8 stream bytes, row}, checks the offsets and
 * reduces the longest stream S; hmj_sort_u64_device sorts them stably; heads, active rows (rows of a segment of several
 * rows with stream bytes left) and active segments are ballots, one scan and one read-back.  A refinement round compacts the
 * active rows, order_refine_kernel gathers their next b = (64 - s) / 8 stream bytes under the s bits of their segment's
 * rank (4 <= b <= 8), one stable sort orders all segments at once, and the rows go back to their positions.  Resolved rows
 * are never read or written again.  At most 1 + ceil(max(0, S - 8) / 4) rounds; a call that has active rows left then is
 * HMJ_E_HIP ("refinement did not converge").
 * Known cost: a long prefix shared by many strings costs one round per 4..8 bytes over the rows that share it (no
 * per-segment common-prefix skip); every round is a full hmj_sort_u64_device call on its rows.
 * Out of scope: 32-bit-offset strings (LIMIT / OFFSET: hmj_top_k_device below), collations and locale, decimal128, host-resident columns, the
 * exchange path.                                                                                                        */
#define HMJ_ORDER_LARGE_STRING 16u /* a column type beside HMJ_TYPE_I8 ... HMJ_TYPE_F64: Arrow large_string              */
#define HMJ_ORDER_DESC        0x1u /* descending among the valid values                                                  */
#define HMJ_ORDER_NULLS_FIRST 0x2u /* NULL slots before every valid value (default: after)                               */
#define HMJ_MAX_ORDER_COLS 8
typedef struct {
  uint32_t type;            /* HMJ_TYPE_* or HMJ_ORDER_LARGE_STRING                                                      */
  uint32_t flags;           /* HMJ_ORDER_* bits; any other bit: HMJ_E_ARG                                                */
  const void* data;         /* fixed: n values aligned to their width; string: chars (NULL legal when all lengths are 0) */
  const uint64_t* offsets;  /* string: n + 1 non-decreasing offsets, offsets[0] need not be 0; fixed: NULL               */
  hmj_validity validity;    /* bits == NULL: no NULL in the column; any bit_offset                                       */
} hmj_order_col;
typedef struct {
  uint32_t struct_size;     /* size-versioned like the other opts                                                        */
  uint32_t reserved;        /* 0                                                                                         */
  uint64_t n_distinct;      /* out: distinct key tuples (0 when n == 0)                                                  */
  uint64_t n_tied_rows;     /* out: rows whose whole key equals another row's                                            */
  uint32_t n_rounds;        /* out: sort rounds run (0 when n <= 1)                                                      */
  uint32_t reserved2;       /* 0                                                                                         */
  float ms_key, ms_sort, ms_refine, ms_map; /* out, with hmj_set_profiling                                               */
} hmj_order_opts;
int hmj_order_by_device(hmj_ctx* ctx, const hmj_order_col* cols, uint32_t n_cols, uint64_t n, uint64_t* row_map_out,
                        hmj_order_opts* opts);

/* ---- window functions over ordered partitions (OVER) ------------------------------------------------------ */
/* A value for EVERY row that depends on the row's neighbours in an ordered partition: up to HMJ_MAX_WINDOW_FNS functions --
 * ROW_NUMBER, RANK, DENSE_RANK, running COUNT / SUM / MIN / MAX, LAG and LEAD -- over one OVER (PARTITION BY keys[0 ..
 * n_partition_cols) ORDER BY the rest of keys) clause, in one call.  Every other entry answers with one row per group or
 * with a row map.  "Top 3 per group" is ROW_NUMBER here followed by hmj_filter_device on the output column (the top k of the
 * whole table is hmj_top_k_device).  Nothing in the reference corresponds.  A new entry with
 * structs of its own: no other entry, struct, flag or path bit changes.
 * keys is a HOST array of n_keys entries, 0 <= n_keys <= HMJ_MAX_ORDER_COLS, exactly what hmj_order_by_device takes; fns
 * and dst are HOST arrays of n_fns entries (read during the call only; dst[a].null_count is written); everything they point
 * to is on the device and caller-owned.  n is at most 2^32 - 1.
 * Order.  The rows are ordered by all keys under hmj_order_by_device's rule: stable, ties keep ascending row index, so the
 * order is total and every output is a function of the inputs alone.  n_keys == 0 is the identity order: one partition of
 * all rows, and no sort runs.  n_partition_cols == n_keys gives partitions whose rows keep the input's order (pandas'
 * groupby(k).cumsum()).  HMJ_ORDER_DESC / HMJ_ORDER_NULLS_FIRST on a partition column only decide where the partitions lie in
 * the map.
 * Partitions and peers.  Two rows are in one partition when they are equal in every partition column under the ORDER BY's
 * own equality: two NULL slots are equal; every NaN is one value; -0.0 and +0.0 differ; strings are equal in length and
 * bytes.  Rows that this equality joins are exactly the rows the sort leaves next to each other, so a partition is one
 * contiguous run of sorted positions.  Peers are rows of one partition that are equal in every order column under the same
 * rule; without order columns a whole partition is one peer group.
 * Output layout.  Slot j of every output belongs to the row at sorted position j, row row_map_out[j]: the outputs are
 * written coalesced, in partition order.  row_map_out is caller-owned device memory of n uint64, aligned to 8, required
 * when n > 0.  Other columns are lined up with the outputs by a take through row_map_out.  A caller who wants the input's
 * row order takes the outputs through the inverse map, which is hmj_order_by_device on row_map_out as one HMJ_TYPE_U64
 * column.  dst[a].validity != NULL: ceil(n / 64) 64-bit words are written exactly as hmj_agg_dst's (slot j = bit j & 63 of
 * word j >> 6, padding bits 0).  dst[a].null_count is filled with or without a bitmap.  The value bytes of a NULL slot are 0.
 * Frame.  The cumulative functions use ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW: the partition's first row through
 * this row.  That is NOT SQL's default RANGE frame: peers do not share a value.
 * Values.  Validity, sign and zero extension, wrapping 64-bit integer sums and float sums in double follow
 * hmj_group_agg_device word for word, and so do MIN / MAX: in the source type and signedness, floats in IEEE order with
 * -0.0 < +0.0, a NaN losing against any number, a prefix whose valid values are all NaN giving the canonical quiet NaN.
 * CUM_SUM / CUM_MIN / CUM_MAX are NULL until the partition's first valid value.  CUM_COUNT is never NULL; its data may be
 * NULL.  ROW_NUMBER, RANK and DENSE_RANK read no source: data, type beyond being a known one, validity and offset are
 * ignored.  LAG / LEAD: the slot is NULL when the position `offset` rows away lies outside the partition or the source slot
 * there is NULL; offset is any uint64, 0 is the row itself, and j + offset is never formed where it could wrap.  A partition
 * boundary resets every carry by selection: a NaN or an infinity of one partition never reaches another, nothing is
 * multiplied away.
 * Float sums are deterministic as hmj_group_agg_device's: the same inputs give the same bits whatever ran before on the ctx
 * and whatever other functions share the call.  The order of the additions is fixed by sorted position in a fixed shape (a
 * segmented scan inside chunks of 64 positions, the chunks of a wave's 512 positions in ascending order, the waves'
 * aggregates in tiles of 2048 -- 8 per lane, a wave scan, the waves in order --, the tiles' totals the same way); there is
 * no atomic on a value.  |got - exact| <= gamma_k * sum|x| over the prefix, gamma_k = k u / (1 - k u), u = 2^-53, k the
 * prefix's valid count, as for any bracketing.
 * Context.  The call has a workspace of its own.  The order comes from hmj_order_by_device on row_map_out, and the call
 * shares that entry's effects and nothing more: a prepared build side is discarded; the lifetime of the last JOIN result
 * ends where a sort runs; what the sorts learn is kept under signature kind 25; hmj_last_plan / hmj_last_timing are left
 * alone; the group result and the live grouping are kept.  It returns with the work complete on the ctx stream.
 * opts (out): n_partitions, n_peer_groups, max_partition_rows (the longest partition); n_rounds of the internal ORDER BY
 * (0 where none ran); with hmj_set_profiling ms_order (the ORDER BY), ms_heads (heads, their carry and the positions'
 * state), ms_scan (every function's launches).
 * n == 0: HMJ_OK, the counters and null counts are 0, nothing is written on the device, and no argument that is only
 * checked with n > 0 is looked at.
 * HMJ_E_ARG, found by the host before any launch (hmj_last_error names what was wrong): NULL ctx / fns / dst / opts; NULL
 * keys with n_keys > 0; n_keys > HMJ_MAX_ORDER_COLS; n_partition_cols > n_keys; opts->struct_size smaller than through
 * `reserved`; non-zero reserved; n_fns outside 1..HMJ_MAX_WINDOW_FNS; an unknown op or type; more than 2^32 - 1 rows; with
 * n > 0: NULL or misaligned source data of a function that reads values (CUM_SUM / CUM_MIN / CUM_MAX / LAG / LEAD), NULL or
 * misaligned dst[a].data, a dst[a].validity not aligned to 8, NULL or misaligned row_map_out, bit_offset + n overflowing 64
 * bits, a destination range (data, bitmap, map) that overlaps a source column, a key column, a bitmap or another
 * destination (address ranges).  Everything hmj_order_by_device rejects in keys is HMJ_E_ARG in that entry's wording, its
 * device-found offset errors included.  The ctx stays usable after any error.
 * How (DESIGN.md "Window functions over ordered partitions").  window_heads_kernel: a wave walks 8 chunks of 64 sorted
 * positions, a lane compares rows map[j] and map[j - 1] column by column (validity, then value; strings by length, then
 * bytes) -- a row's fixed-width keys are gathered once, by the lane of its position, and reach the lane above by __shfl_up
 * --, the ballots of "partition head" and "peer head" are one word each per chunk, partitions and peer
 * groups are counted by popcount (one atomic per workgroup), and the wave stores one aggregate of the positions' state.
 * window_carry_kernel scans the waves' aggregates -- four slots of {accumulator, valid count, saw a head}, a head selecting
 * the right operand -- in tiles, and once more over the tiles' totals; window_state_kernel gives every chunk its
 * {partitions in front, dense rank carried in, last partition head, last peer head} and finds the longest partition.
 * window_rank_kernel, up to 4 functions per launch: ROW_NUMBER, RANK and DENSE_RANK from that state and the two words,
 * LAG / LEAD by comparing the partition of position j -+ offset and one gather.  window_scan_kernel, up to 4 functions per
 * launch, runs twice: a wave walks its 8 chunks, loads the map entry and the head word once for all functions, issues every
 * gather before the segmented __shfl_up scan and stores its aggregates; behind the carry the same walk starts from the
 * carried value and writes the outputs, a bitmap word per ballot, NULLs counted by popcount.  One read-back of the counters.
 * Known cost: the cumulative functions gather their sources twice; window_heads_kernel reads both neighbours' strings whole.
 * Out of scope: RANGE and sliding frames; NTILE / PERCENT_RANK / FIRST_VALUE / LAST_VALUE; string-valued LAG / LEAD;
 * whole-partition aggregates (group, aggregate, then a take through group_of_row); the exchange path, host-resident
 * columns.                                                                                                              */
#define HMJ_WIN_ROW_NUMBER 0u  /* -> uint64, 1-based position in the partition; never NULL; reads no source               */
#define HMJ_WIN_RANK       1u  /* -> uint64, ROW_NUMBER of the first row of this row's peer group                          */
#define HMJ_WIN_DENSE_RANK 2u  /* -> uint64, peer groups of the partition up to and including this row's                   */
#define HMJ_WIN_CUM_COUNT  3u  /* -> uint64, valid source values from the partition's first row through this row           */
#define HMJ_WIN_CUM_SUM    4u  /* -> int64 / uint64 / double, as HMJ_AGG_SUM                                               */
#define HMJ_WIN_CUM_MIN    5u  /* -> the source type, as HMJ_AGG_MIN                                                       */
#define HMJ_WIN_CUM_MAX    6u
#define HMJ_WIN_LAG        7u  /* -> the source type: the value `offset` rows earlier in the partition                     */
#define HMJ_WIN_LEAD       8u  /* ... `offset` rows later                                                                   */
#define HMJ_MAX_WINDOW_FNS 32
typedef struct {
  const void* data;       /* device: n values of `type`, aligned to their width; NULL legal where the op reads no value */
  uint32_t type;          /* HMJ_TYPE_*                                                                              */
  uint32_t op;            /* HMJ_WIN_*                                                                               */
  hmj_validity validity;  /* source bitmap, any bit_offset; bits == NULL: the column has no NULL                     */
  uint64_t offset;        /* HMJ_WIN_LAG / HMJ_WIN_LEAD: rows away; any value                                        */
} hmj_window_fn;
typedef struct {
  void* data;             /* device, caller-owned: n values of the function's output type, aligned to it             */
  uint64_t* validity;     /* device, caller-owned, or NULL: ceil(n / 64) 64-bit words, padding bits written as 0     */
  uint64_t null_count;    /* out: NULL slots of this output column (filled with or without bitmap)                   */
} hmj_window_dst;
typedef struct {
  uint32_t struct_size;        /* size-versioned like the other opts                                                 */
  uint32_t n_partition_cols;   /* in: the first n_partition_cols of keys are PARTITION BY, the rest ORDER BY         */
  uint64_t n_partitions, n_peer_groups, max_partition_rows;  /* out                                                  */
  uint32_t n_rounds;           /* out: hmj_order_opts.n_rounds of the internal ORDER BY (0 where none ran)           */
  uint32_t reserved;           /* 0                                                                                  */
  float ms_order, ms_heads, ms_scan;  /* out, with hmj_set_profiling                                                 */
} hmj_window_opts;
int hmj_window_device(hmj_ctx* ctx, const hmj_order_col* keys, uint32_t n_keys, uint64_t n,
                      const hmj_window_fn* fns, uint32_t n_fns, hmj_window_dst* dst,
                      uint64_t* row_map_out, hmj_window_opts* opts);

/* ---- the first rows of an order: ORDER BY ... LIMIT k [OFFSET o] (top-k) ---------------------------------------- */
/* Entries offset .. offset + k of the map hmj_order_by_device returns for the same columns, without sorting the rows the cut
 * rejects: "the ten largest sums" reads the key column a few times and sorts ten rows.  Nothing in the reference
 * corresponds.  A new entry with structs of its own: no other entry, struct, flag or path bit changes.
 * Result.  row_map_out[j], j < n_out, equals entry offset + j of hmj_order_by_device's map of cols: the order is total and
 * stable (ties keep ascending row index), so the answer is unique and every plan returns the same entries.  Entries from
 * n_out on are not written.  cols is exactly what hmj_order_by_device takes (a HOST array of n_cols entries, everything
 * behind it on the device), and the value rules -- directions, NULL placement, integers, floats, NaN, strings -- are that
 * entry's word for word.  n is at most 2^32 - 1; k and offset are any uint64.
 * Offset arithmetic.  offset + k saturates: the cut is K = min(n, offset + k) and n_out = min(k, n - min(n, offset)),
 * computed without wrapping for any pair of values.
 * Empty results.  n_out == 0 -- k == 0, offset >= n or n == 0 --: HMJ_OK, nothing is written, no kernel is launched,
 * plan_taken = 0, the ctx is as it was.  The host argument checks still run, except those hmj_order_by_device makes only
 * with n > 0.  row_map_out is required when n_out > 0, must then be aligned to 8, and its 8 * n_out bytes must not overlap a
 * column's values, offsets or bitmap.  n == 1 with n_out == 1: the map is {0}; no column is read, no kernel runs
 * (plan_taken = 0, n_candidates = 1).
 * Plans.  HMJ_TOPK_SELECT: a radix selection over the rows' byte streams finds the K-th row's place without materialising
 * the rows it rejects; the candidates -- every row before the cut, and the rows still tied with it -- are ordered by
 * hmj_order_by_device's own refinement loop.  HMJ_TOPK_FULL: hmj_order_by_device into a workspace map, then the slice.
 * HMJ_TOPK_AUTO takes FULL where selection cannot pay: n below 2^23 rows, or K above n / 256 (DESIGN.md records where these
 * come from).  max_tie_rows: a set of rows tied with the cut that is larger than this is narrowed by a further level before
 * it is ordered; 0 is the library's default (2^14).
 * Context.  The effects are hmj_order_by_device's and nothing more: a prepared build side is discarded; the lifetime of the
 * last JOIN result ends where a sort runs (a call whose candidates are one row sorts nothing); hmj_last_plan /
 * hmj_last_timing are left alone; the group result and the live grouping are kept; the sorts learn under signature kind
 * 25.  The call has a workspace of its own beside hmj_order_by_device's, runs on the ctx stream and returns with the map
 * complete.
 * opts (out): n_out; n_candidates -- rows the final ordering sorted (SELECT: K <= n_candidates <= n; FULL: n); n_tie_rows --
 * rows still tied with the cut when selection stopped, before trimming (0 where the whole tie set lies before the cut);
 * plan_taken; n_levels -- histogram levels run (0 under FULL); n_rounds -- sort rounds of the final ordering; with
 * hmj_set_profiling ms_select (the first window's levels), ms_emit (marks, writes and every later window), ms_order (the
 * final ordering and the slice; under FULL the whole ORDER BY).
 * HMJ_E_ARG, found by the host before any launch: NULL ctx / cols / opts; an unknown plan; non-zero reserved;
 * opts->struct_size smaller than through `max_tie_rows`; a NULL, misaligned or overlapping row_map_out with n_out > 0; and
 * everything hmj_order_by_device rejects in cols, in that entry's wording.  Found on the device by the first kernel that
 * computes a stream, before any kernel follows an offset into chars, again in that entry's wording: decreasing offsets, and
 * key bytes of a valid slot under data == NULL.  The ctx stays usable after any error.
 * How (DESIGN.md "Top-k (ORDER BY ... LIMIT)").  A row's order is the memcmp order of its stream (above); selection walks
 * it one 8-byte window at a time.  A LEVEL (topk_hist_kernel, one lane per row) counts the rows whose word agrees with
 * the threshold prefix decided so far into an LDS histogram of the next 11-bit digit -- a wave whose lanes share one bin
 * adds their popcount once, a workgroup flushes its non-zero bins with one global atomic each --, the host reads the bins
 * back and picks the digit that holds the K-th row: the rows in smaller bins are definite, the bin is the new tie set.  The
 * call's first level also makes hmj_order_by_device's offset checks and reduces the longest stream and the bits in which
 * the words differ, so that later digits start at the highest varying bit.  Selection stops when the tie set is at most
 * max_tie_rows, when all of it lies before the cut, or when the window's bits are used up.  topk_mark_kernel ballots
 * "below the threshold" and "tied", one scan places both, topk_write_kernel writes {first stream word, row} of the rows
 * below, then of the tied rows, each class in ascending row order: rows of equal whole keys share a class, so the stable
 * sorts behind keep them in row order.  Tied rows whose stream is used up are equal in every column: only the first of
 * them by row index that the cut takes are written (ORDER BY status LIMIT 10 sorts ten rows).  Tied rows with bytes left
 * and more than max_tie_rows of them become a list; its next 8 stream bytes are gathered and the same levels, marks and
 * writes run over the list, window by window.
 * Known cost: the final ordering also refines ties that lie wholly behind the cut; every level is one launch and one
 * read-back, and reads the key columns (window 0) or the list's words again; FULL and a SELECT whose candidates are most
 * of the table cost an ORDER BY plus the levels.
 * Out of scope: WITH TIES; top-k per partition (ROW_NUMBER and hmj_filter_device); pruning the refinement behind the cut;
 * 32-bit-offset strings; the exchange path; host-resident columns.                                                     */
#define HMJ_TOPK_AUTO   0u   /* the library chooses */
#define HMJ_TOPK_SELECT 1u   /* radix selection, then the candidates are ordered */
#define HMJ_TOPK_FULL   2u   /* the full ORDER BY into a workspace map, then the slice */
typedef struct {
  uint32_t struct_size;   /* size-versioned like the other opts */
  uint32_t plan;          /* in: HMJ_TOPK_*; exists so callers and tests can pin a path (as force_hashed does) */
  uint64_t offset;        /* in: rows skipped in front (OFFSET) */
  uint64_t max_tie_rows;  /* in: 0 = the library's default; a tie set larger than this is narrowed by a further level */
  uint64_t n_out;         /* out: map entries written = min(k, n - min(n, offset)) */
  uint64_t n_candidates;  /* out: rows the final ordering sorted (SELECT: K <= n_candidates <= n; FULL: n) */
  uint64_t n_tie_rows;    /* out: rows still tied with the cut when selection stopped, before trimming */
  uint32_t plan_taken;    /* out: HMJ_TOPK_SELECT / HMJ_TOPK_FULL; 0 where no kernel ran */
  uint32_t n_levels;      /* out: histogram levels run (0 under FULL) */
  uint32_t n_rounds;      /* out: sort rounds of the final ordering */
  uint32_t reserved;      /* 0 */
  float ms_select, ms_emit, ms_order; /* out, with hmj_set_profiling */
} hmj_top_k_opts;
int hmj_top_k_device(hmj_ctx* ctx, const hmj_order_col* cols, uint32_t n_cols, uint64_t n, uint64_t k,
                     uint64_t* row_map_out, hmj_top_k_opts* opts);

/* ---- taking fixed-width columns through a row map (Arrow validity out) --------------------------------- */
/* The joins above return gather maps (r_row / s_row), not columns.  This entry turns a map back into Arrow columns: up to
 * HMJ_MAX_TAKE_COLS fixed-width columns of ONE relation (n_src rows each; keys, payloads, anything of 1, 2, 4, 8 or 16
 * bytes per value) are taken through row_map (n_out entries) into caller-owned output columns, each with an optional
 * validity bitmap and always with its null count.  src and dst are HOST arrays of n_cols entries (read during the call
 * only; dst[c].null_count is written); everything they point to is on the device.
 * Output slot i of column c is NULL when row_map[i] == HMJ_TAKE_NO_ROW (an outer join's missing partner), or when source
 * row row_map[i] is NULL in column c (src[c].validity, an Arrow bitmap at any bit_offset; bits == NULL: the column has no
 * NULL).  Otherwise it is valid and its value is the source value bit for bit.  The value bytes of a NULL output slot are
 * written as 0, whatever lies under the source's NULL slot: the output is a function of the inputs alone.
 * dst[c].validity != NULL: ceil(n_out / 64) 64-bit words are written, an Arrow bitmap at bit offset 0 (row i = bit i & 63
 * of word i >> 6, least-significant bit first, which is Arrow's byte order on a little-endian host); the padding bits
 * behind row n_out - 1 are written as 0.  dst[c].null_count is filled with or without a bitmap.  A map without
 * HMJ_TAKE_NO_ROW over sources without bitmaps gives all-ones bitmaps (padding 0) and null_count 0.  opts->n_no_row: the
 * map entries equal to HMJ_TAKE_NO_ROW.
 * row_map may be a column the ctx owns -- the last result's r_row / s_row of hmj_join_cols_device,
 * hmj_join_kind_cols_device, hmj_join_mixed_device, hmj_join_str_device or hmj_join_kind_str_device -- or any device array
 * of the caller's.  The
 * call neither releases nor overwrites the last result and does not discard a prepared build side; its only workspace is
 * a small counter buffer of its own.  hmj_last_plan, hmj_last_timing and the workload memos stay as they were.  It returns
 * with the work complete on the ctx stream, like the joins; the counts come back to the host.
 * A map entry >= n_src that is not HMJ_TAKE_NO_ROW is HMJ_E_ARG, and hmj_last_error says how many there were.  The kernel
 * compares before it loads, so such an index is never dereferenced (its lane writes a NULL slot); the outputs are
 * unspecified after the error and the ctx stays usable.
 * HMJ_E_ARG also (hmj_last_error names what was wrong): NULL ctx / src / dst / opts; a NULL row_map with n_out > 0;
 * opts->struct_size smaller than through `reserved`; non-zero reserved (opts or a column); n_cols outside
 * 1..HMJ_MAX_TAKE_COLS; a width other than 1, 2, 4, 8 or 16; NULL or misaligned data (source when n_src > 0, destination
 * when n_out > 0; a 16-byte column is aligned to 16); a row_map or dst validity pointer not aligned to 8 bytes; bit_offset +
 * n_src overflowing 64 bits; n_out or n_src above 2^32-1; a destination range (data or bitmap) that overlaps the row map or
 * any source column or source bitmap of the call (a host check on address ranges).
 * n_out == 0 returns HMJ_OK and writes nothing on the device.  n_src == 0 is legal when every entry is HMJ_TAKE_NO_ROW
 * (source pointers may then be NULL).
 * How (DESIGN.md "Taking columns through a join's row maps"): cols_take_kernel, one lane per output row in 256-thread
 * workgroups, up to 8 columns per launch (the host loops over chunks of 8).  The map entry is loaded once per row and tested
 * once for all columns; all of a row's gathers are issued before its first store.  A wave covers 64 consecutive rows that
 * start at a multiple of 64, so its ballot of "valid" is one bitmap word, stored by one lane: no atomics and no
 * read-modify-write on the bitmap.  The counts are ballot popcounts, one atomic per workgroup and counter.
 * Out of scope: host-resident columns, bit-packed boolean value columns, the exchange path.  Variable-width (string)
 * columns go through hmj_take_str_device below.                                                                      */
#define HMJ_TAKE_NO_ROW UINT64_MAX   /* == HMJ_COLS_NO_ROW == HMJ_STR_NO_ROW */
#define HMJ_MAX_TAKE_COLS 64
typedef struct {
  const void* data;       /* device: n_src values of `width` bytes, aligned to `width`          */
  uint32_t width;         /* 1, 2, 4, 8 or 16                                                    */
  uint32_t reserved;      /* 0                                                                   */
  hmj_validity validity;  /* source bitmap, any bit_offset; bits == NULL: the column has no NULL */
} hmj_take_src;
typedef struct {
  void* data;             /* device, caller-owned: n_out * width bytes, aligned to width         */
  uint64_t* validity;     /* device, caller-owned, or NULL: ceil(n_out / 64) 64-bit words; Arrow
                             bitmap at bit offset 0, row i = bit i, padding bits written as 0    */
  uint64_t null_count;    /* out: NULL slots of this output column (filled with or without bitmap) */
} hmj_take_dst;
typedef struct {
  uint32_t struct_size;   /* size-versioned like the other opts                                  */
  uint32_t reserved;
  uint64_t n_no_row;      /* out: map entries equal to HMJ_TAKE_NO_ROW                           */
  float ms_take;          /* out, with hmj_set_profiling                                         */
} hmj_take_opts;
int hmj_take_cols_device(hmj_ctx* ctx, const hmj_take_src* src, uint32_t n_cols, uint64_t n_src,
                         const uint64_t* row_map, uint64_t n_out, hmj_take_dst* dst, hmj_take_opts* opts);

/* ---- taking an Arrow string column through a row map --------------------------------------------------- */
/* The sibling of hmj_take_cols_device for ONE variable-width column per call: an Arrow large_string / large_binary column
 * (n_src rows: n_src + 1 64-bit offsets into a chars buffer, an optional validity bitmap) is taken through row_map (n_out
 * entries) into caller-owned offsets, chars and an optional validity bitmap, in the same contract style: what turns the
 * r_row / s_row of the string joins (and the string key columns of hmj_join_mixed_device) back into their key strings,
 * or takes any other string column of either relation.  src,
 * dst and opts are host structs; everything they point to is on the device.
 * NULL and empty slots.  Output slot i is NULL when row_map[i] == HMJ_TAKE_NO_ROW or source row row_map[i] is NULL
 * (src->validity, any bit_offset; bits == NULL: no NULL).  A NULL slot has length 0, whatever bytes the source holds under
 * its NULL slot; a valid empty string is valid with length 0.  The offsets of a source slot that is NULL or never taken are
 * not consulted: they may hold anything.  Source offsets[0] need not be 0, and src->chars needs no alignment.
 * Sizing and full calls.  dst->chars == NULL is the sizing call: it writes dst->offsets (n_out + 1 final values,
 * offsets[0] = 0), the bitmap (when dst->validity != NULL: ceil(n_out / 64) words as hmj_take_dst's, padding bits 0),
 * dst->null_count, dst->total_bytes (= offsets[n_out]) and opts->n_no_row, and copies no bytes.  With dst->chars set the
 * call does all of that and copies the bytes: a caller who knows an upper bound needs one call, otherwise two.  If
 * chars_capacity < total_bytes the call returns HMJ_E_ARG with dst->total_bytes filled, and not one byte of chars is
 * written.
 * Outputs.  Offsets, bitmap words and counts are a function of the inputs alone.  Exactly the bytes chars[0, total_bytes)
 * are written: no byte at or behind total_bytes changes, although the kernel stores 16 bytes at a time (the last, short
 * piece is stored bytewise).
 * Bad map entries and bad source offsets are HMJ_E_ARG, never a fault: a map entry >= n_src that is not HMJ_TAKE_NO_ROW,
 * and a taken valid row with offsets[r + 1] < offsets[r] or offsets[r + 1] > chars_bytes; hmj_last_error gives the counts.
 * All three are compared before any address is formed from them; such a lane contributes a NULL slot of length 0, and the
 * bytes phase does not run.  The outputs are unspecified after the error and the ctx stays usable.
 * HMJ_E_ARG also, found on the host before any launch (hmj_last_error names what was wrong): NULL ctx / src / dst / opts;
 * opts->struct_size smaller than through `reserved`, non-zero reserved; a NULL row_map or NULL dst->offsets with n_out > 0;
 * NULL source offsets with n_src > 0; NULL source chars with chars_bytes > 0; a row_map, source offsets, dst->offsets or
 * dst->validity not aligned to 8 bytes, or dst->chars not aligned to 16; n_out or n_src above 2^32-1; bit_offset + n_src
 * overflowing 64 bits; a destination range -- offsets, bitmap words, chars[0, chars_capacity) -- that overlaps the row map,
 * the source offsets, the source bitmap, [chars, chars + chars_bytes) or another destination range of the call (address
 * ranges; ranges that merely touch do not overlap).
 * n_out == 0 is HMJ_OK with total_bytes = 0, and nothing on the device is written (not even offsets[0]).  Like
 * hmj_take_cols_device the call keeps the last result, a prepared build side, hmj_last_plan, hmj_last_timing and the workload
 * memos as they were -- its only workspace is a counter block and the per-workgroup byte totals with their scan --; row_map
 * may be the ctx's own r_row / s_row; it returns with the work complete on the ctx stream.
 * How (DESIGN.md "Taking string columns through a join's row maps").  Offsets phase: one lane per output row, one
 * 256-thread workgroup per 256 consecutive rows; the map entry is tested once, offsets[r], offsets[r + 1] and the validity
 * byte are gathered together, the row is checked; a wave's ballot of "valid" is one bitmap word, the counts are ballot
 * popcounts; the workgroup's exclusive scan of the lengths goes to dst->offsets, the workgroup totals are scanned, and a
 * streaming kernel adds every workgroup's base and writes offsets[n_out].  The host reads one counter block back: the only
 * synchronisation before the bytes phase, and where a bad call stops.  Bytes phase, balanced by output bytes: a workgroup
 * owns a tile of 4096 output bytes, finds the rows that intersect it by binary search in the final offsets and stages
 * their output and source starts in LDS (up to 1024 rows per tile; beyond, lanes read them from global memory); a lane
 * builds one aligned 16-byte piece from aligned 16-byte source granules that hold a byte of a taken row, shifted into
 * place, and stores it once.  A row longer than a tile is covered by several tiles.
 * opts->ms_offsets / ms_chars: HIP-event times of the two phases with hmj_set_profiling (ms_chars 0 for a sizing call). */
typedef struct {
  const void* chars;        /* device; may be NULL when chars_bytes == 0; need not be aligned        */
  uint64_t chars_bytes;     /* size of the chars buffer: no taken row may end behind it               */
  const uint64_t* offsets;  /* device: n_src + 1 offsets, Arrow large_string; offsets[0] need not be 0 */
  hmj_validity validity;    /* source bitmap at any bit_offset; bits == NULL: no NULL                 */
} hmj_take_str_src;
typedef struct {
  uint64_t* offsets;        /* device, caller-owned: n_out + 1 entries, offsets[0] = 0                */
  void* chars;              /* device, caller-owned, aligned to 16; NULL: a sizing call               */
  uint64_t chars_capacity;  /* bytes available behind chars                                           */
  uint64_t* validity;       /* device or NULL: ceil(n_out / 64) words, as hmj_take_dst                */
  uint64_t null_count;      /* out */
  uint64_t total_bytes;     /* out: offsets[n_out], filled by sizing and full calls alike             */
} hmj_take_str_dst;
typedef struct { uint32_t struct_size, reserved; uint64_t n_no_row; float ms_offsets, ms_chars; } hmj_take_str_opts;
int hmj_take_str_device(hmj_ctx* ctx, const hmj_take_str_src* src, uint64_t n_src, const uint64_t* row_map,
                        uint64_t n_out, hmj_take_str_dst* dst, hmj_take_str_opts* opts);

/* ---- filtering rows: typed and string predicates to a row map (WHERE) ---------------------------------- */
/* Selection: a predicate in conjunctive normal form over up to HMJ_MAX_FILTER_TERMS terms -- each one column, one
 * comparison and its literal(s) -- is evaluated at n input positions, and the positions at which it is TRUE come back as
 * a row map, the one hmj_take_cols_device and hmj_take_str_device consume, with an optional Arrow bitmap of the same
 * fact.  Every term reads its column either directly (position i reads row i) or through a row map of its own, so a
 * predicate behind a join names columns of R through r_row and columns of S through s_row in one call:
 * `... FULL OUTER JOIN ... WHERE s.key IS NULL` is one IS_NULL term through s_row.  Nothing in the reference corresponds.
 * A new entry with structs of its own: no other entry, struct, flag or path bit changes.
 * terms is a HOST array of n_terms entries (read during the call only); everything a term points to is on the device,
 * except the string literals (host pointers, copied by the call).  n is at most 2^32 - 1.
 * Outputs.  row_map_out: caller-owned device memory of n uint64, aligned to 8; exactly opts->n_out entries are written,
 * the passing positions in ascending order (the compaction is stable); no entry at or behind n_out is written.  mask_out:
 * a device pointer aligned to 8, or NULL; when set, ceil(n / 64) words are written, an Arrow bitmap at bit offset 0 whose
 * bit i is 1 when position i passes, padding bits 0, exactly as hmj_take_dst's.  opts (out): n_out; n_unknown -- the
 * positions whose predicate is UNKNOWN (the FALSE count is n - n_out - n_unknown); with hmj_set_profiling ms_eval (the
 * evaluation and the scan) and ms_write (the map).
 * A term.  type: HMJ_TYPE_I8 ... HMJ_TYPE_F64 (data: n_src values aligned to their width) or HMJ_FILTER_LARGE_STRING
 * (data: the chars, chars_bytes of them; offsets: n_src + 1 64-bit offsets, offsets[0] need not be 0).  validity: any
 * bit_offset; bits == NULL: the column has no NULL.  row_map: NULL -- position i reads row i, and n_src >= n --, or n
 * entries on the device -- position i reads row row_map[i], HMJ_TAKE_NO_ROW is a NULL slot --; the maps may be the ctx's
 * own result columns.  op: HMJ_FILTER_EQ, NE, LT, LE, GT, GE, BETWEEN (closed, two literals), IS_NULL, IS_NOT_NULL and, on
 * strings only, STARTS_WITH and ENDS_WITH.  flags: HMJ_FILTER_NOT.  clause: terms of one clause are ORed, the clauses are
 * ANDed; clause ids must not decrease along terms; an IN-list is a clause of EQ terms.  Literals: a fixed column's are
 * lit[0] (and lit[1] for BETWEEN), the value's bits in the column's own type in the low bytes -- no casts are performed,
 * and bits that do not fit the width are HMJ_E_ARG --; a string column's are str_lit[k] / str_len[k], host pointers (NULL
 * with length 0 is the empty string), at most HMJ_MAX_FILTER_LITERAL_BYTES over all terms of a call.  The literals of
 * IS_NULL / IS_NOT_NULL are not looked at.
 * Semantics.  Three-valued logic: a comparison on a NULL slot is UNKNOWN; IS_NULL and IS_NOT_NULL are never UNKNOWN;
 * HMJ_FILTER_NOT swaps TRUE and FALSE and leaves UNKNOWN; OR is the maximum and AND the minimum under FALSE < UNKNOWN <
 * TRUE; a position passes only when the whole predicate is TRUE.  Integers compare in their own signedness.  Floats
 * compare as C's operators do, which is IEEE: -0.0 == +0.0, and a NaN on either side makes every comparison FALSE except
 * NE, which is TRUE -- deliberately NOT the total order of hmj_order_by_device (there -0.0 < +0.0 and NaN is one value
 * above +inf): a caller who writes `x = 0.0` wants both zeros.  BETWEEN lo, hi is lo <= x && x <= hi (lo > hi selects
 * nothing).  Strings compare as std::string::operator< does: unsigned bytes, then length -- the ORDER BY rule; NUL and
 * bytes >= 0x80 are ordinary bytes; a NULL string is not the empty string; STARTS_WITH "" is TRUE for every valid slot.
 * What lies under a NULL slot is never read: value bytes, string bytes and the offsets of that row.
 * Errors, all HMJ_E_ARG (hmj_last_error names what was wrong; the ctx stays usable).  Found on the host before any
 * launch: NULL ctx / terms / opts; n_terms outside 1..HMJ_MAX_FILTER_TERMS; an unknown type, op or flag bit; a string-only
 * op on a fixed column; decreasing clause ids; non-zero reserved fields, opts->struct_size smaller than through
 * `reserved2`; NULL or misaligned data, offsets, row_map, row_map_out or mask_out where n > 0 needs them (chars need no
 * alignment and may be NULL when chars_bytes is 0; offsets on a fixed column); bit_offset + n_src overflowing 64 bits; n
 * or n_src above 2^32 - 1; n_src < n without a map; a literal that does not fit its width; literal bytes over the cap; an
 * output range (map or mask) that overlaps any input range of the call or the other output (address ranges, as the takes
 * check them).  Found on the device, and never a fault: a map entry >= n_src that is not HMJ_TAKE_NO_ROW, and a read
 * valid string row with offsets[r + 1] < offsets[r] or offsets[r + 1] > chars_bytes; each is compared before any address is
 * formed from it, such a lane counts as UNKNOWN, the write phase does not run, and hmj_last_error gives the counts.  The
 * outputs are unspecified after an error.  n == 0 is HMJ_OK with nothing written on the device.
 * Context.  The takes' rules, because the maps may be the live result's own: the call keeps the last join result, a
 * prepared build side, the group result, the live grouping, hmj_last_plan, hmj_last_timing and the workload memos; its
 * workspace is its own, kept on the ctx, grown on demand and released by hmj_destroy; it returns with the work complete
 * on the ctx stream.
 * How (DESIGN.md "Filtering rows (WHERE)").  filter_eval_kernel: one lane per position in blocks of 256 positions that
 * start at multiples of 256; a 256-thread workgroup walks 8 consecutive blocks, 4 at a time, so that a lane has 4 loads
 * in flight at every step; the terms are kernel arguments, the string literals sit in LDS, the term list is unrolled
 * for 1, 2, 4, 8 or 16 terms; a lane loads each distinct map's entry once (the first four distinct maps; a term on a
 * later one loads its own), walks the terms with a running clause maximum and predicate minimum, and the wave's ballot of
 * TRUE is one mask word (to mask_out, or to the workspace); TRUE and UNKNOWN popcounts go to a slot per block, the
 * error counters take one atomic per workgroup.  A two-level scan of the slots (no workgroup waits on another), one
 * counter read-back, then filter_write_kernel ranks every set bit of the mask words inside its block, adds the
 * block's base and stores the position.
 * Out of scope: LIKE / CONTAINS / regular expressions, column-to-column comparisons, casts, decimal128, 32-bit-offset
 * strings, host-resident columns, the exchange path.                                                                  */
#define HMJ_FILTER_LARGE_STRING 16u /* == HMJ_ORDER_LARGE_STRING: a column type beside HMJ_TYPE_I8 ... HMJ_TYPE_F64        */
#define HMJ_FILTER_EQ 0u
#define HMJ_FILTER_NE 1u
#define HMJ_FILTER_LT 2u
#define HMJ_FILTER_LE 3u
#define HMJ_FILTER_GT 4u
#define HMJ_FILTER_GE 5u
#define HMJ_FILTER_BETWEEN 6u      /* lit[0] <= x && x <= lit[1]                                                          */
#define HMJ_FILTER_IS_NULL 7u
#define HMJ_FILTER_IS_NOT_NULL 8u
#define HMJ_FILTER_STARTS_WITH 9u  /* strings only                                                                        */
#define HMJ_FILTER_ENDS_WITH 10u   /* strings only                                                                        */
#define HMJ_FILTER_NOT 0x1u        /* hmj_filter_term.flags: swaps TRUE and FALSE, leaves UNKNOWN                         */
#define HMJ_MAX_FILTER_TERMS 16
#define HMJ_MAX_FILTER_LITERAL_BYTES 4096
typedef struct {
  uint32_t type;            /* HMJ_TYPE_* or HMJ_FILTER_LARGE_STRING                                                     */
  uint32_t op;              /* HMJ_FILTER_EQ ... HMJ_FILTER_ENDS_WITH                                                    */
  uint32_t flags;           /* HMJ_FILTER_NOT; any other bit: HMJ_E_ARG                                                  */
  uint32_t clause;          /* terms of one clause are ORed, clauses ANDed; never decreasing along terms                 */
  const void* data;         /* fixed: n_src values aligned to their width; string: chars (NULL legal with chars_bytes 0) */
  const uint64_t* offsets;  /* string: n_src + 1 offsets, offsets[0] need not be 0; fixed: NULL                          */
  uint64_t chars_bytes;     /* string: size of the chars buffer, no read row may end behind it; fixed: ignored           */
  hmj_validity validity;    /* bits == NULL: no NULL in the column; any bit_offset                                       */
  uint64_t n_src;           /* rows of the column                                                                        */
  const uint64_t* row_map;  /* NULL: position i reads row i; else n entries, HMJ_TAKE_NO_ROW is a NULL slot              */
  uint64_t lit[2];          /* fixed: the literal's bits in the column's type, low bytes ([1]: BETWEEN's upper bound)    */
  const void* str_lit[2];   /* string: HOST pointers to the literal bytes (NULL with length 0: the empty string)         */
  uint64_t str_len[2];
  uint64_t reserved;        /* 0                                                                                         */
} hmj_filter_term;
typedef struct {
  uint32_t struct_size;     /* size-versioned like the other opts                                                        */
  uint32_t reserved;        /* 0                                                                                         */
  uint64_t n_out;           /* out: positions at which the predicate is TRUE = entries written to row_map_out            */
  uint64_t n_unknown;       /* out: positions at which the predicate is UNKNOWN                                          */
  float ms_eval, ms_write;  /* out, with hmj_set_profiling                                                               */
  uint64_t reserved2;       /* 0                                                                                         */
} hmj_filter_opts;
int hmj_filter_device(hmj_ctx* ctx, const hmj_filter_term* terms, uint32_t n_terms, uint64_t n, uint64_t* row_map_out,
                      uint64_t* mask_out, hmj_filter_opts* opts);

/* Host threads of the optional staged upload (pageable input -> pinned chunks -> PCIe), used only
 * with HMJ_UPLOAD=staged in the environment; by default each relation goes up in one copy straight
 * from the caller's memory (54 GB/s on the MI355X box).  The reference ctor's num_threads argument,
 * hashjoin.h:58, maps to this.  Default min(8, cores).                                            */
int hmj_set_host_threads(hmj_ctx* ctx, int n);

/* ---- multi-GPU: the radix partition exchange --------------------------------------- */
/* One process per GPU, one ctx per process.  The reference reaches all of its parallelism from the ctor
 * (hashjoin.h:56-68 -> radix_hash.h:375-405: fork-join over threads of one address space); this is the same
 * fork-join over GPUs: every rank passes its row shard of R and S, the ranks exchange rows so that each owns
 * a disjoint set of keys (radix fan-out over ranks; partition p of the probe side only ever meets table p,
 * hashjoin_bench.cc:92-96), and each joins what it owns.
 *
 * Communicator.  RCCL over xGMI: rank 0 makes an id (hmj_comm_unique_id), the host program hands the 128 bytes
 * to every rank by whatever it has (torch.distributed, MPI, a file), every rank calls hmj_comm_init_rank.
 * librccl is loaded at the first of these calls (dlopen: the library itself does not link it; a process that
 * already holds RCCL, e.g. through PyTorch, shares that copy).  Alternatively the host supplies the two
 * collectives itself (hmj_comm_set_transport): an existing communicator, or -- as the tests do -- several
 * ranks on one GPU over gloo.  Both are collective calls: all ranks, same order.                           */
#define HMJ_UNIQUE_ID_BYTES 128
int hmj_comm_unique_id(void* id128);
int hmj_comm_init_rank(hmj_ctx* ctx, int n_ranks, int rank, const void* id128);
typedef struct hmj_transport {
  void* user;
  int n_ranks, rank;
  /* both callbacks return 0 = ok, HMJ_E_TIMEOUT = gave up waiting for a peer (the step then returns HMJ_E_TIMEOUT and
   * the communicator is marked unusable), anything else = failed (HMJ_E_RCCL).
   * every rank contributes `count` values; recv[r * count + i] = rank r's send[i].  Host memory, blocking.  */
  int (*allgather_u64)(void* user, const uint64_t* send, uint64_t* recv, int count);
  /* one round of the all-to-all-v on DEVICE memory: send send_bytes[g] bytes at send_ptrs[g] to rank g and
   * receive recv_bytes[g] bytes from it into recv_ptrs[g] (g == own rank: a local copy).  hip_stream
   * (hipStream_t): the inputs are complete on it and the received bytes must be usable by later work on it
   * -- queue the transfers there, or synchronise it, move the data and return.  0 = ok.                      */
  int (*alltoallv)(void* user, int round, const void* const* send_ptrs, const uint64_t* send_bytes,
                   void* const* recv_ptrs, const uint64_t* recv_bytes, void* hip_stream);
} hmj_transport;
int hmj_comm_set_transport(hmj_ctx* ctx, const hmj_transport* t);
int hmj_comm_destroy(hmj_ctx* ctx); /* also done by hmj_destroy */
/* Message sizes (0 = leave unchanged).  max_message_bytes: no single send exceeds it (default and maximum
 * 2^30: RCCL 2.26 truncates a message of 2 GiB or more); a bucket larger than that goes in rounds.
 * probe_round_bytes: target size of a probe-side message (default 128 MiB): the probe side travels in several
 * rounds so that the local partitioning starts on the rows that have arrived.                              */
int hmj_comm_set_message_bytes(hmj_ctx* ctx, uint64_t max_message_bytes, uint64_t probe_round_bytes);
/* The deadline of ONE hmj_exchange_join_u64_device call, in milliseconds from its start (default 120 000, or
 * HMJ_COMM_TIMEOUT_MS in the environment when the communicator is created; 0 = wait for ever).  The reference's
 * workers all return from the one call that started them (hashjoin.h:56-68 -> radix_hash.h:375-405: pthread_join);
 * ranks in different processes can lose a peer, so every wait of a step that depends on another rank -- the
 * all-gathers, the build side's rounds, each probe round -- is a host-side poll (hipEventQuery / hipStreamQuery +
 * ncclCommGetAsyncError) under this deadline, and a watchdog thread covers a host blocked inside RCCL itself (it calls
 * ncclCommAbort, which is what makes such a call return).  When the deadline passes the call returns HMJ_E_TIMEOUT, and
 * so does every later step on this communicator: hmj_comm_destroy it (that is where a communicator whose stream is still
 * busy is aborted -- RCCL's kernels leave their wait loops, the stream drains -- instead of destroyed) and make a new one
 * (all ranks).  Each rank notices on its own -- there is nobody left to tell
 * it -- so a step ends everywhere within the deadline plus about a second.  Callback transports must bound their own
 * waits by the same number (hmj_comm_get_timeout_ms) and return HMJ_E_TIMEOUT from the callback.  Not during a step. */
int hmj_comm_set_timeout_ms(hmj_ctx* ctx, uint64_t timeout_ms);
int hmj_comm_get_timeout_ms(hmj_ctx* ctx, uint64_t* timeout_ms);

/* The distributed join.  Replaces the HashMergeJoin ctor + iteration (hashjoin.h:56-68, :183-191) for
 * relations sharded by rows over the ranks.  The radix fan-out itself is the owner (round 3): every rank runs the
 * FIRST radix pass of the join on its own shards -- stable histogram / scan / scatter on the top `digit_bits` key
 * bits under the prefix all ranks' keys share (the window is agreed through one all-gather of key samples), exactly
 * pass 1 of the reference's sort (radix_hash.h:313-345, top-bits routing radix_hash.h:369) -- and rank g owns a
 * contiguous RANGE of those digits, chosen from the pooled sample so that the ranks balance.  The digit-major rows
 * then travel in rounds of digit sub-ranges (grouped send/recv on the communicator's own stream; build side first);
 * a round that has arrived is a complete key range of both relations and is joined at once by the remaining
 * radix passes + build + probe, while later rounds are still on the links.  Nothing is partitioned twice.
 * Fallbacks: a key sample whose digits cannot be balanced over the ranks (a few clusters of keys) selects the
 * hash owner floor(mix64(key) * n_ranks / 2^64) with a separate owner split (round 2's path, even for any key
 * set); HMJ_ORDERED uses key-range owners between splitters = quantiles of the pooled sample, so rank g's ordered
 * rows precede rank g+1's and the concatenation in rank order is the reference's iteration order.
 * HMJ_FIRST_WINS is global when rank r's build shard precedes rank r+1's in input order (rows are received
 * source-major inside a round and every pass is stable).
 * local_out: this rank's result (materialising flags: columns are device pointers owned by the ctx; count modes:
 * the sums over the key ranges this rank owns).  global_out (may be NULL): counts and checksums over all ranks,
 * columns NULL.  Collective: all ranks, same flags; an error on one rank (bad sizes, out of memory, a failed
 * local join) makes EVERY rank return -- the failing one its own code, the others HMJ_E_PEER -- instead of
 * leaving its peers blocked in the next collective.  One rank: the plain local join (nothing to exchange),
 * unless hmj_comm_set_self_exchange asked for the whole path.
 * STATUS: the digit-owner path (round 3, the default for non-ordered joins) has been verified with several ranks
 * sharing one GPU over the callback transport and with one rank over RCCL; it has NOT yet run over RCCL between
 * two real GPUs (no such box was available).  hmj_comm_set_owner_path(ctx, HMJ_OWNER_SPLIT) -- or
 * HMJ_EXCHANGE_OWNER=split in the environment when the communicator is created -- selects round 2's owner-split
 * path (hash owner, separate split, ONE local join) for all non-ordered joins instead.                         */
int hmj_exchange_join_u64_device(hmj_ctx* ctx, const void* build_shard_dev, uint64_t n_build_shard,
                                 const void* probe_shard_dev, uint64_t n_probe_shard, uint32_t flags,
                                 hmj_result* local_out, hmj_result* global_out);
/* One-rank communicators only (tests, rehearsals on a one-GPU box): on != 0 runs the whole exchange -- digit
 * pre-pass, rounds through the transport (RCCL self send/recv), per-round joins -- where the default is the plain
 * local join.                                                                                                */
int hmj_comm_set_self_exchange(hmj_ctx* ctx, int on);
/* Which owner function non-ordered distributed joins use (collective setting: the same on every rank).
 * HMJ_OWNER_DIGIT (default): ranges of the first radix pass's digit, per-round joins.  HMJ_OWNER_SPLIT: the hash
 * owner with its separate owner split and one local join -- the path every clustered key set falls back to anyway.
 * Nothing in the reference corresponds (one address space, radix_hash.h:375-405).                              */
#define HMJ_OWNER_DIGIT 0
#define HMJ_OWNER_SPLIT 1
int hmj_comm_set_owner_path(hmj_ctx* ctx, int owner_path);
/* The owner split on its own: rows grouped by owner rank, stably (owner-major; within an owner in input
 * order), offsets_dev[g] = first row of owner g (2^ceil(log2 n_ranks) + 1 uint64, device).  splitters: NULL =
 * hash owner; else n_ranks - 1 ascending keys (host memory) = key-range owner.  in/out must not overlap.   */
int hmj_owner_split_u64_device(hmj_ctx* ctx, const void* in_aos_dev, uint64_t n, int n_ranks,
                               const uint64_t* splitters, void* out_aos_dev, uint64_t* offsets_dev);
typedef struct {
  int n_ranks, owner_mode;            /* owner_mode: 1 = hash of the key, 2 = key ranges (splitters),          */
                                      /* 3 = ranges of the first radix pass's digit, 0 = one rank, no exchange */
  uint32_t rounds_build, rounds_probe;
  uint64_t recv_build, recv_probe;    /* rows this rank owns                                                */
  float ms_split;                     /* digit pre-pass (or owner split) of both shards + the read-back of the */
                                      /* counts (host clock)                                                 */
  float ms_exchange_build, ms_exchange_probe; /* on the communication stream                                */
  float ms_local;                     /* from "build side complete" to the end of the local join(s) (host clock) */
  float ms_total;
  int32_t digit_bits, digit_low;      /* owner_mode 3: digit = (key >> digit_low) & (2^digit_bits - 1)         */
  uint32_t n_subjoins;                /* local joins run (one per round of the digit path)                     */
  uint32_t fallback;                  /* 1: the digit owner was rejected (sample not balanceable): hash owner  */
  float sample_max_share;             /* owner_mode 3: largest sampled share of a rank x n_ranks (1 = even)    */
  float ms_kernels;                   /* device time of this rank's own kernels in the step (pre-pass + local  */
                                      /* joins; HIP events, needs hmj_set_profiling)                           */
  float ms_exposed;                   /* ms_total - ms_kernels: what the exchange and its synchronisation added */
} hmj_exchange_info;
int hmj_last_exchange_info(hmj_ctx* ctx, hmj_exchange_info* out);
/* Digit-range owners and rounds, exported because they are pure host arithmetic (no GPU needed; every rank
 * computes the same plan from the same pooled key sample).  sample_keys: the pooled sample (any order).
 * digit = (key >> digit_low) & (2^digit_bits - 1): the top <= 8 bits under the prefix all sampled keys share.
 * owner_first[g] .. owner_first[g+1]: the digits rank g owns (boundaries where the sample's cumulative count is
 * closest to g / n_ranks); round_first[g][r] .. [r+1]: the digits of rank g that travel in round r.
 * usable = 0: fewer than 2 digits per rank, or the fullest rank would get more than 1.3 x its share.          */
#define HMJ_MAX_RANKS 16
#define HMJ_MAX_ROUNDS 16
typedef struct {
  int32_t usable;
  int32_t digit_bits, digit_low;
  uint32_t n_rounds;
  uint32_t owner_first[HMJ_MAX_RANKS + 1];
  uint32_t round_first[HMJ_MAX_RANKS][HMJ_MAX_ROUNDS + 1];
  float max_share;
} hmj_digit_plan;
int hmj_exchange_digit_plan(int n_ranks, const uint64_t* sample_keys, uint64_t n_sample, uint32_t n_rounds,
                            hmj_digit_plan* out);
/* One relation's messages under a digit plan.  counts[src * 2^digit_bits + d] = rows of digit d in rank src's
 * shard.  For round r and peer g (index r * n_ranks + g): rows [send_off, +send_rows) of this rank's digit-major
 * buffer go to g; rows [recv_off, +recv_rows) of its receive buffer are filled by g.  The receive buffer is
 * round-major, inside a round source-major (sources in rank order = global input order): round r occupies rows
 * [round_off[r], round_off[r+1]) and is a complete key range once every source's message has arrived.        */
int hmj_exchange_digit_layout(int n_ranks, int rank, const hmj_digit_plan* plan, const uint64_t* counts,
                              uint64_t* send_off, uint64_t* send_rows, uint64_t* recv_off, uint64_t* recv_rows,
                              uint64_t* round_off);
/* The round plan of the owner-split path (hash / key-range owners), exported because it is pure host arithmetic
 * (no GPU needed; every rank computes the same from the same count matrix).  counts[src * n_ranks + dst] = rows rank src sends to rank dst.
 * hmj_exchange_rounds: rounds so that no message exceeds max_msg_rows.  hmj_exchange_layout: for round r and
 * peer g (index r * n_ranks + g) the rows [send_off, +send_rows) of this rank's owner-major split buffer that
 * go to g, and the rows [recv_off, +recv_rows) of its receive buffer that g's message fills.  layout 0 =
 * source-major (a source's rows contiguous, sources in rank order = global input order), 1 = round-major
 * (a round's rows contiguous; round_end[r] = rows complete after round r).                                  */
uint32_t hmj_exchange_rounds(int n_ranks, const uint64_t* counts, uint64_t max_msg_rows);
int hmj_exchange_layout(int n_ranks, int rank, const uint64_t* counts, uint32_t n_rounds, int layout,
                        uint64_t* send_off, uint64_t* send_rows, uint64_t* recv_off, uint64_t* recv_rows,
                        uint64_t* round_end);

/* ---- one radix pass ---------------------------------------------------------------------------- */
/* Replaces pass 1 of radix_int_non_inplace / radix_non_inplace_par: per-worker histogram, exclusive
 * scan partition-major/worker-minor, STABLE scatter (radix_sort.h:418-449, radix_hash.h:313-345) on
 * digit = (key >> shift) & (2^bits - 1), 1 <= bits <= 9.  offsets_dev: 2^bits + 1 uint64 bucket
 * starts (device).  in/out: n x {key,val}, device, must not overlap.  Also the multi-GPU owner
 * split.                                                                          */
int hmj_partition_u64_device(hmj_ctx* ctx, const void* in_aos_dev, uint64_t n, int shift, int bits,
                             void* out_aos_dev, uint64_t* offsets_dev);

/* ---- full radix sort ------------------------------------------------------------ */
/* Replaces radix_int_non_inplace<uint64_t,uint64_t>(begin, end, dst, num_threads)
 * (radix_sort.h:452-522) -- the call radix_bench_par.cc:126-127 times: rows sorted by key, ascending,
 * out of place.  From 2^22 rows on (out != in): MSD, as the reference's own sort is (radix_hash.h:202-292) -- two
 * histogram-free slab passes on the top 12 ... 18 varying key bits, every partition sorted on the remaining bits in LDS
 * (HMJ_PATH_SORT_MSD: 3 x 32 B per row whatever the key width); otherwise, or where the keys crowd into few partitions:
 * stable LSD passes over the 8-bit digits in which keys differ (write-combining scatter; from 2^25 rows on
 * histogram-free slab passes chained one into the next + one compaction).  Equal keys keep their
 * input order in every form (the reference is stable in pass 1 only, so on duplicate keys its payload order may
 * differ; the key column and the multiset of rows are identical).  in/out: n x {key,val}, device.
 * out == in sorts in place -- the replacement of radix_int_inplace<uint64_t,uint64_t>(begin, n,
 * num_threads) (radix_sort.h:333-398; radix_bench_par.cc:96), which is unstable: same key column, same
 * multiset of rows.  A partial overlap of in and out is not allowed.                               */
int hmj_sort_u64_device(hmj_ctx* ctx, const void* in_aos_dev, uint64_t n, void* out_aos_dev);

/* Replaces radix_hash::radix_inplace_par on a caller's pre-hashed tuple buffer (radix_hash.h:589-654) -- what the
 * HashMergeJoin2 ctor does to BOTH relations as a side effect callers may rely on (hashjoin.h:234-235): n rows
 * of row_bytes bytes in HOST memory are sorted IN PLACE, ascending on the uint64 at byte offset key_offset.
 * Stable (equal keys keep their input order; the reference's swap chains are not).  The rows go to the GPU,
 * {key, index} pairs are sorted there (eight 8-bit LSD passes), the rows are gathered and copied back.
 * row_bytes: a multiple of 8 in 16..64 (std::tuple<size_t, uint64_t, uint64_t> is 24; libstdc++ stores the
 * elements in reverse order, so its hash sits at offset 16).                                               */
int hmj_sort_rows_by_u64_host(hmj_ctx* ctx, void* rows_host, uint64_t n, uint32_t row_bytes, uint32_t key_offset);
/* The sorted order only, for rows the GPU cannot move (non-trivial types such as std::string keys): key i is the
 * uint64 at keys_host + i * stride_bytes; perm_out[j] = input index of the row that belongs at position j.   */
int hmj_argsort_u64_host(hmj_ctx* ctx, const void* keys_host, uint64_t n, uint32_t stride_bytes, uint32_t* perm_out);

/* ---- synthetic relations on device (same integer arithmetic as the oracle) ------- */
/* key = mix64(i + seed), val = i, i in [start, start+n)                                          */
int hmj_gen_build_u64_device(hmj_ctx* ctx, void* out_aos_dev, uint64_t n, uint64_t start,
                             uint64_t seed);
/* j in [start,start+n): idx = (0x9E3779B1*j + 12345) mod n_build (+ n_build when miss_mod > 0 and
 * j % miss_mod == 0); key = mix64(idx + seed); val = j ^ 0x9E3779B97F4A7C15                      */
int hmj_gen_probe_u64_device(hmj_ctx* ctx, void* out_aos_dev, uint64_t n, uint64_t start,
                             uint64_t n_build, uint64_t seed, uint64_t miss_mod);
/* rank = lower_bound(thr_dev[0..domain), mix64(i ^ zseed)); key = mix64(rank + seed); val = i     */
int hmj_gen_from_cdf_u64_device(hmj_ctx* ctx, void* out_aos_dev, uint64_t n, uint64_t start,
                                const uint64_t* thr_dev, uint64_t domain, uint64_t seed,
                                uint64_t zseed);
/* key = mix64((mix64(j ^ zseed) % domain) + seed); val = j ^ 0x9E3779B97F4A7C15                   */
int hmj_gen_uniform_domain_u64_device(hmj_ctx* ctx, void* out_aos_dev, uint64_t n, uint64_t start,
                                      uint64_t domain, uint64_t seed, uint64_t zseed);

#ifdef __cplusplus
}
#endif
#endif /* HMJ_H */
