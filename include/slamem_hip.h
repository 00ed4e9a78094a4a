/* slamem_hip.h -- C ABI of the MI355X-native MEM engine (libslamem_hip.so).
 *
 * Drop-in boundary for slaMEM's MEM path.  The reference has no FFI layer: its
 * boundary is the pair of C headers bwtindex.h + lcparray.h as used by
 * GetMatches (slamem.c:37-218).  Those are per-base calls on file-static
 * globals, unusable across a PCIe/GPU boundary, so the ABI below is the coarse
 * (batched, handle-based, error-code) form of the same operations; every entry
 * point cites the reference interface it replaces.  Plain C types only: no
 * torch / HIP types in any signature (streams are passed as void*).
 *
 * Conventions
 *   - every function returns SLAMEM_OK (0) or a SLAMEM_ERR_* code; nothing
 *     calls exit() (the reference prints to stdout and exit(-1)s:
 *     slamem.c:58-61, bwtindex.c:1441-1444).  slamem_last_error_message()
 *     gives the text for the calling thread.
 *   - "_dev" pointers are device (HBM) pointers on the index's device.
 *   - rows are BWT rows 0..n (n = text length; row 0 is the '$' suffix);
 *     intervals are inclusive [top, bottom], as in the reference.
 *   - coordinates in slamem_mem are 0-based; the CLI prints them 1-based
 *     like slamem.c:148.
 */
#ifndef SLAMEM_HIP_H
#define SLAMEM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAMEM_ABI_VERSION 4

enum {
    SLAMEM_OK = 0,
    SLAMEM_ERR_ARG = 1,      /* bad argument                                     */
    SLAMEM_ERR_HIP = 2,      /* a HIP runtime call failed (message has the text) */
    SLAMEM_ERR_NOMEM = 3,    /* host or device allocation failed                 */
    SLAMEM_ERR_CAPACITY = 4, /* output buffer too small; *total_out has the need */
    SLAMEM_ERR_FORMAT = 5,   /* arena / file is not a slamem index               */
    SLAMEM_ERR_IO = 6,
    SLAMEM_ERR_NO_DEVICE = 7 /* no usable MI355X: there is NO CPU fallback       */
};

typedef struct slamem_index slamem_index; /* opaque; one per device, immutable after build */

/* One MEM: T[ref_pos .. ref_pos+length) == Q[query_pos .. query_pos+length),
 * not extendable on either side.  Replaces the fprintf at slamem.c:148,173. */
typedef struct {
    uint32_t ref_pos;
    uint32_t query_pos; /* in the strand that was scanned (reverse blocks: in the reverse complement, slamem.c:100-102) */
    uint32_t length;
} slamem_mem;

/* One segment of a gapped alignment (option -aln): ref_len letters of the text from ref_pos against query_len
 * letters of the scanned strand from query_pos, with `edits` letters under X, I and D of its CIGAR. */
typedef struct {
    uint32_t ref_pos;
    uint32_t query_pos;
    uint32_t ref_len;
    uint32_t query_len;
    uint32_t edits;
} slamem_aln;

/* One read's mapping (option -paf).  strand: 0 the read is unmapped, 1 its mapping lies on the forward strand,
 * 2 on the reverse strand; mapq: 0 to 60; s1: the score of the primary strand block's best chain; s2: that of the best competing
 * chain. */
typedef struct {
    uint32_t s1;
    uint32_t s2;
    uint8_t strand;
    uint8_t mapq;
    uint8_t reserved[2]; /* 0 */
} slamem_map;

typedef struct {
    uint32_t text_length;  /* n                                           */
    uint32_t bwt_size;     /* n + 1            == FMI_GetBWTSize(), bwtindex.c:263 */
    uint32_t num_n_rows;   /* BWT rows holding 'N'                        */
    uint32_t dollar_row;   /* BWT row holding '$'                         */
    uint32_t max_lcp;      /* largest LCP value                           */
    uint32_t sort_rounds;  /* prefix-doubling rounds the build needed     */
    uint64_t arena_bytes;  /* bytes of HBM the index occupies             */
    int32_t device;
    int32_t owns_arena;
    uint32_t filter_k;     /* k of the k-mer presence filter (0 = the index has none); no reference counterpart */
    uint32_t layout;       /* SLAMEM_LAYOUT_FULL or SLAMEM_LAYOUT_COMPACT: what the build chose (ABI 2: reserved, 0)   */
    uint32_t seed_k;       /* letters of a seed of the seed-and-compare sections (0 = the index has none); ABI 4; no reference counterpart */
    uint32_t reserved1;
} slamem_index_info;

/* Index layouts (no reference counterpart: the reference has one layout of 3.3 B per letter made for CPU caches,
 * bwtindex.c:33-37 + lcparray.c:46-57; here HBM is spent to cut dependent random reads).
 *   FULL     every section: ~37.5 B per text letter + 16-32 B of presence filter + the seed-and-compare sections of the search of
 *            reads (ABI 4: seed table 16-32 B per letter, 8-16 B for texts of 2^28 letters and more -- there only when the build
 *            still fits the free HBM with it --, spill list, the text in 32-byte units): 8.3 GB at 100 Mbp, 188 GB at 3.1 Gbp
 *   COMPACT  no text-ordered sections (the search walks the index where it would have compared with the text) and a
 *            presence filter of half the size: ~21.5 B per letter + 8-16 B (3.3 GB at 100 Mbp, 81 GB at 3.1 Gbp); same
 *            results, slower search (DESIGN.md 2 has the measured cost)
 *   AUTO     FULL when its build peak fits the HBM that is free on the device, else COMPACT, else SLAMEM_ERR_NOMEM with
 *            the numbers in the message.  SLAMEM_INDEX_LAYOUT=full|compact in the environment decides instead;
 *            SLAMEM_HBM_BUDGET_GB caps what counts as free. */
enum { SLAMEM_LAYOUT_AUTO = 0, SLAMEM_LAYOUT_FULL = 1, SLAMEM_LAYOUT_COMPACT = 2 };

/* Per-phase device times of the last build / search on this thread's most recent
 * call, in milliseconds, measured with HIP events on the stream the kernels ran on. */
typedef struct {
    float build_total_ms;
    float build_pack_ms;      /* K1 text pack + histogram                         */
    float build_sort_ms;      /* K2 suffix sort (all radix passes, all rounds)    */
    float build_bwt_ms;       /* K3 BWT planes + rank samples                     */
    float build_lcp_ms;       /* K5 exact LCP                                     */
    float build_links_ms;     /* K7 PSV / NSV                                     */
    float search_kernel_ms;   /* K8a + K8: prefilter, work-list compaction, search */
    float search_total_ms;    /* K8 + scan + K9 scatter                           */
    uint64_t search_launches; /* number of K8 launches accumulated since reset    */
    double search_kernel_ms_sum;
    float prefilter_ms;       /* K8a (work-item fill + presence prefilter), part of search_kernel_ms */
    float k8_ms;              /* K8 k_find_mems_v3 alone, part of search_kernel_ms */
    double prefilter_ms_sum;
    double k8_ms_sum;
    float seed_ms;            /* K8s k_seed_mems (seed-and-compare for reads; runs in K8a's place), part of search_kernel_ms (ABI 4) */
    float mum_filter_ms;      /* -mum / -smem / -chain / -ext / -aln / -paf: the filter behind K9 (mum_filter.hip, smem_filter.hip, chain_filter.hip, ext_filter.hip, aln_filter.hip, map_filter.hip), large blocks included; 0 for -mem and -mam */
    double seed_ms_sum;
} slamem_timings;

/* Load counters of ONE diagnostic search launch (slamem_search_stats_enable): how many loads of each kind the lanes of
 * K8a / K8 issued.  The diagnostic launch runs separate kernel instantiations that carry the counters; the normal
 * (timed) kernels carry none.  "lines" are 64-byte lines: FM blocks are one line each, a row-record pair is one or two.
 * bench.py prices roofline.traffic from these (cross-checked against the rocprofv3 PMC pass kept under profiles/). */
typedef struct {
    uint64_t fm_lines_top;          /* K8: FM block of `top` fetched (one per backward step unless still in registers) */
    uint64_t fm_lines_bottom;       /* K8: FM block of `bottom+1` when it is a different block                         */
    uint64_t rec_lines_fail;        /* K8: row-record lines after a failed extension (parent step)                     */
    uint64_t rec_lines_pend;        /* K8: row-record lines for the exact parent depth of a pending position           */
    uint64_t rec_lines_flush;       /* K8: row-record lines at strand ends                                             */
    uint64_t query_loads;           /* K8: 32-byte query windows loaded                                                */
    uint64_t lane_trips;            /* K8: loop trips summed over active lanes                                         */
    uint64_t wave_trips;            /* K8: loop trips summed over waves (lane_trips / (64 * wave_trips) = lane use)    */
    uint64_t positions;             /* K8: query positions consumed                                                    */
    uint64_t enum_jobs;             /* K8: wave-cooperative enumeration jobs                                           */
    uint64_t prefilter_probes;      /* K8a: presence-filter lines fetched (the tests behind a hit read the same line)  */
    uint64_t prefilter_query_loads; /* K8a: 16-byte query loads                                                        */
    uint64_t prefilter_items;       /* K8a: work items screened                                                        */
    uint64_t items;                 /* work items of the batch                                                         */
    uint64_t survivors;             /* work items K8 scanned                                                           */
    uint64_t mems;                  /* MEMs found                                                                      */
    uint64_t overflow_records;      /* MEMs that went through the atomic overflow list                                 */
    uint64_t valid;                 /* 1 when the counters describe a launch                                           */
    uint64_t dir_sa_lines;          /* K8 direct extension: suffix-array lines (one per run)                           */
    uint64_t dir_group_loads;       /* K8 direct extension: text groups (16 letters + classes, 16 B) with 16 B of query */
    uint64_t dir_rec_lines;         /* K8 direct extension: text-ordered records (one per run)                         */
    uint64_t dir_letters;           /* K8 direct extension: query positions consumed by comparing with the text        */
    uint64_t jump_lines;            /* K8: K-mer jump table entries read (one per scan start)                          */
    uint64_t skip_group_loads;      /* K8 skipping: text groups read to verify the diagonal behind a disagreeing letter */
    uint64_t skip_probe_lines;      /* K8 skipping: words of the k-mer occurrence bitmap read                          */
    uint64_t skip_attempts;         /* K8 skipping: diagonals verified (probes follow)                                 */
    uint64_t skips;                 /* K8 skipping: stretches skipped (min_len positions each)                         */
    uint64_t enum_row_steps;        /* K8: wave steps of the enumeration jobs (64 rows tested for left-maximality each)  */
    uint64_t enum_levels;           /* K8: ancestor intervals the enumeration jobs walked up to (one record round trip each) */
    uint64_t enum_wave_us;          /* K8: microseconds the waves spent inside enumeration jobs, summed over waves (compare k8 wave sum) */
    /* K8: loop trips per state of the lane's state machine (EXT, REC, FLUSH, DSA, DIR, DEND, JQ, JT, SKV, SKQ, SKP): summed
     * over lanes, and the number of WAVE trips in which at least one lane was in the state (what the wave pays for) */
    uint64_t state_lane_trips[11];
    uint64_t state_wave_trips[11];
    /* K8s (ABI 4): seed-and-compare for reads */
    uint64_t seed_windows;          /* K8s: seed-table lines fetched (one 64-byte line per window looked up; both strands share it)    */
    uint64_t seed_compares;         /* K8s: diagonals compared with the text (four 32-byte units of the text each: 128 bytes)          */
    uint64_t seed_letter_masks;     /* K8s: compares whose text units hold a letter that is not A,C,G,T                               */
    uint64_t seed_mems;             /* K8s: MEMs it reported                                                                          */
    uint64_t seed_strands_left;     /* K8s: strands left to the index walk (K8)                                                       */
    uint64_t seed_reads;            /* K8s: reads screened                                                                            */
    uint64_t seed_query_bytes;      /* K8s: bytes of the reads it packed                                                              */
    /* K8s: events counted on the way: [0] reads left to K8 before any lookup (longer than the kernel's strands, a letter that is
     * not A,C,G,T; also the reads of a wave whose compares did not fit), [1] windows whose bucket holds more k-mers than the
     * table keeps (28), [2] palindromic windows that hit (compared on both strands: not left), [3] trips whose compares did not
     * fit, [4] inconsistent hits (never), [5] MEMs beyond the wave's list, [6] MEMs whose tie with another of their strand (same
     * start, same length) the text behind them does not decide                                                                  */
    uint64_t seed_left_why[7];
    uint64_t seed_once_reads;       /* K8s: compares of the first round (they also look at the occurs-once plane of their units)    */
} slamem_search_stats;

/* ---- library ---------------------------------------------------------- */
int slamem_abi_version(void);
const char *slamem_strerror(int code);
const char *slamem_last_error_message(void);
int slamem_device_count(int *count_out);
/* Creates the HIP context of `device` (runtime start-up takes ~0.2 s): a front end calls this from a helper thread
 * while it parses its input, so that the index build does not pay for it.  No reference counterpart. */
int slamem_device_warmup(int device);
/* PCI address of `device` ("0000:c1:00.0"): a front end reads /sys/bus/pci/devices/<address>/local_cpulist to keep its host
 * threads on the GPU's NUMA node.  No reference counterpart. */
int slamem_device_pci_bus_id(int device, char *out, int out_bytes);
/* Free and total HBM of `device` in bytes (hipMemGetInfo): a front end that starts right behind another GPU job waits
 * for the memory its index needs (slamem_index_build_bytes) instead of failing.  No reference counterpart. */
int slamem_device_mem_info(int device, uint64_t *free_out, uint64_t *total_out);
int slamem_get_timings(slamem_timings *out);
int slamem_reset_timings(void);
/* on != 0: the NEXT slamem_find_mems_device calls of this thread run the diagnostic kernel instantiations (same results,
 * slower) and slamem_get_search_stats returns the counters of the last one.  No reference counterpart. */
int slamem_search_stats_enable(int on);
int slamem_get_search_stats(slamem_search_stats *out);
/* Timeline of the same diagnostic launch of K8 (device wall clock): microseconds from the first wave's start until the
 * work list was empty, microseconds from then until the last wave left (the tail), and the sum of all waves' run times. */
int slamem_get_search_clock(double *us_to_empty_list, double *us_tail, double *us_wave_sum);

/* ---- (a) index construction ------------------------------------------- */
/* Replaces FMI_BuildIndex(texts,sizes,1,&lcp,verbose) (bwtindex.h:7, call at
 * slamem.c:73) followed by BuildSampledLCPArray(text,n,lcp,minlcp,verbose)
 * (lcparray.h:1, call at slamem.c:74).  text: n bytes of A,C,G,T,N (any case;
 * every other byte counts as N, as letterIds does at bwtindex.c:183-196).
 * The text is borrowed for the call only (the reference frees it right after
 * the build too, slamem.c:75-77).  Everything runs on the device: suffix sort,
 * BWT bit-planes + rank samples, exact LCP, PSV/NSV links. */
int slamem_index_build(const char *text_host, uint32_t n, int device, slamem_index **out);
int slamem_index_build_device(const void *text_dev, uint32_t n, int device, void *stream, slamem_index **out);
/* The same with the layout stated (SLAMEM_LAYOUT_*; the two entry points above pass SLAMEM_LAYOUT_AUTO). */
int slamem_index_build_layout(const char *text_host, uint32_t n, int device, int layout, slamem_index **out);
int slamem_index_build_device_layout(const void *text_dev, uint32_t n, int device, void *stream, int layout,
                                     slamem_index **out);
/* HBM a text of n letters takes in `layout` (SLAMEM_LAYOUT_FULL / _COMPACT): the arena that stays, and the peak while
 * it is built (arena + suffix-sort scratch).  Host arithmetic only. */
int slamem_index_build_bytes(uint32_t n, int layout, uint64_t *arena_bytes_out, uint64_t *peak_bytes_out);
/* Replaces FMI_FreeIndex() + FreeSampledSuffixArray() (slamem.c:208-209). */
int slamem_index_free(slamem_index *idx);
int slamem_index_get_info(const slamem_index *idx, slamem_index_info *out);

/* The index is ONE contiguous HBM arena (4 KiB header + arrays), so that it can
 * be broadcast to peer GPUs with a single RCCL call and saved / loaded as one
 * blob (the reference only has a commented-out IDX0 sketch, bwtindex.c:480-579). */
int slamem_index_arena(const slamem_index *idx, void **arena_dev_out, uint64_t *bytes_out);
int slamem_index_export(const slamem_index *idx, void *dst_dev, uint64_t dst_bytes, void *stream);
/* Borrow an arena that a peer built (after ncclBroadcast / torch.distributed.broadcast).
 * The caller keeps the memory alive until slamem_index_free(). */
int slamem_index_attach(void *arena_dev, uint64_t bytes, int device, slamem_index **out);
/* Hand the attached arena over to the handle: slamem_index_free() will hipFree it (it must come from hipMalloc). */
int slamem_index_adopt_arena(slamem_index *idx);
int slamem_index_save(const slamem_index *idx, const char *path);
int slamem_index_load(const char *path, int device, slamem_index **out);
/* Host-only check of the first bytes (>= 256) of an arena or index file against the bytes available: magic, version, and
 * every section offset / size the kernels will index (aligned, ordered, inside the arena).  load and attach run the
 * same check; a corrupt or truncated index is SLAMEM_ERR_FORMAT, never a GPU fault. */
int slamem_index_validate_header(const void *header, uint64_t header_bytes, uint64_t available_bytes);

/* Structure-level parity (all uniquely defined by the text).
 * which: one of SLAMEM_ARRAY_*; host_dst must hold count elements of the stated type. */
enum {
    SLAMEM_ARRAY_SA = 0,  /* uint32[n+1]  suffix array                                  */
    SLAMEM_ARRAY_BWT = 1, /* uint8[n+1]   letter ids $=0 N=1 A=2 C=3 G=4 T=5            */
    SLAMEM_ARRAY_LCP = 2, /* int32[n+2]   exact LCP, [0] = [n+1] = -1                   */
    SLAMEM_ARRAY_PSV = 3, /* uint32[n+2]  nearest smaller value above (valid for 1..n)  */
    SLAMEM_ARRAY_NSV = 4  /* uint32[n+2]  nearest smaller value below (valid for 1..n)  */
};
int slamem_index_download(const slamem_index *idx, int which, void *host_dst, uint64_t count);

/* What the reference's sampled structure (SSILCP, lcparray.c:46-57) WOULD hold for this text, computed on the
 * device from the per-row records: the quantities BuildSampledLCPArray prints (lcparray.c:709-711, 999-1000).
 *   sample        = BWT row i with LCP[i] != LCP[i+1]                        (lcparray.c:677-678)
 *   oversized lcp = sample whose value is -1 or >= 255                       (lcparray.c:688-697)
 *   link          = top corner (LCP[i+1] > LCP[i]): PSV[i];  bottom corner: NSV[i+1]-1   (lcparray.c:827-912)
 *   oversized link= |distance| >= 128, plus the first and the last sample    (lcparray.c:755, 840, 890, 966-970)
 * Used by the front end to print the reference's statistics lines and by the tests as a check of rows a9-a11. */
typedef struct {
    uint64_t num_samples;
    uint64_t num_oversized_lcp;
    int64_t sum_lcp;            /* sum over rows 1..n+1 (the last one counts -1), lcparray.c:668 */
    uint32_t max_lcp;
    uint32_t pad;
    uint64_t num_oversized_links;
    uint64_t sum_link_distance;
    uint64_t max_link_distance;
} slamem_sslcp_stats;
int slamem_index_sampled_lcp_stats(const slamem_index *idx, slamem_sslcp_stats *out);

/* ---- fine-grained operations, batched (one lane per element) ------------ */
/* FMI_FollowLetter (bwtindex.h:8 / bwtindex.c:359): in-place on top/bottom; size_out[i] = new
 * interval size or 0 (then top/bottom are left unchanged). */
int slamem_follow_letter_batch(const slamem_index *idx, const char *letters_dev, uint32_t *top_dev,
                               uint32_t *bottom_dev, uint32_t *size_out_dev, uint64_t count, void *stream);
/* GetEnclosingLCPInterval (lcparray.h:2 / lcparray.c:330): in-place; depth_out[i] = parent depth, -1 at the root. */
int slamem_enclosing_interval_batch(const slamem_index *idx, uint32_t *top_dev, uint32_t *bottom_dev,
                                    int32_t *depth_out_dev, uint64_t count, void *stream);
/* FMI_PositionInText (bwtindex.h:9 / bwtindex.c:402). */
int slamem_position_in_text_batch(const slamem_index *idx, const uint32_t *rows_dev, uint32_t *pos_out_dev,
                                  uint64_t count, void *stream);
/* FMI_GetCharAtBWTPos (bwtindex.h:10 / bwtindex.c:304): one of "$NACGT". */
int slamem_char_at_bwt_pos_batch(const slamem_index *idx, const uint32_t *rows_dev, char *chars_out_dev,
                                 uint64_t count, void *stream);

/* ---- (b) MEM retrieval ---------------------------------------------------- */
/* Replaces the query loop of GetMatches (slamem.c:90-207) for a BATCH of query
 * records: per record the forward strand and, if both_strands, its reverse
 * complement (ReverseComplementSequence, sequence.c:413) are scanned right to
 * left with backward search + parent-interval widening, and every MEM of
 * length >= min_len is reported.
 *
 *   queries_dev       concatenated query characters (A,C,G,T,N; other bytes = N);
 *                     16-byte aligned and readable up to the next multiple of 16 bytes
 *   offsets_dev       uint64[num_queries+1]; record i is [offsets[i], offsets[i+1])
 *   query_bytes       offsets[num_queries] (total characters; sizes the work-item tables: records longer than 4096
 *                     characters are cut into slices that different lanes scan)
 *   strand blocks     block b = 2*i + strand when both_strands, else b = i
 *   mems_dev          out: slamem_mem[mems_capacity], grouped by block, inside a
 *                     block in the reference's emission order (slamem.c:139-193)
 *   block_offsets_dev out: uint64[num_blocks+1]; block b owns [off[b], off[b+1])
 *   workspace_dev     scratch of slamem_find_mems_workspace_bytes() bytes
 *   total_out         number of MEMs found (also when SLAMEM_ERR_CAPACITY is returned)
 *   limit             a strand (or a 4096-position slice of a long one) may emit fewer than 2^28 MEMs: beyond that the call
 *                     fails with SLAMEM_ERR_ARG and says so (never wrong output)
 *   passes            a batch of reads is answered in one pass with one host round trip (the total).  The call does not look
 *                     at the record lengths first: when the batch turns out to hold a record of more than 4096 letters (it
 *                     needs slices) the work is done again with the item tables -- two passes, same answer
 *
 * Synchronous with respect to the stream on return (it has to read the total). */
int slamem_find_mems_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes,
                                     uint64_t mems_capacity, uint64_t *bytes_out);
int slamem_find_mems_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            slamem_mem *mems_dev, uint64_t mems_capacity, uint64_t *block_offsets_dev,
                            void *workspace_dev, uint64_t workspace_bytes, void *stream, uint64_t *total_out);

/* The same batch in MAM mode (option -mam: matchType 1, slamem.c:131,657): only positions whose match is a single
 * BWT row are reported.  The reference skips the other positions with a `continue` that also skips its interval
 * bookkeeping (slamem.c:197-198), which makes later fall-backs start from a stale interval; the
 * result is defined by that behaviour and is reproduced exactly.  Same arguments, layout and errors as
 * slamem_find_mems_device; strands are scanned whole (one lane per strand). */
int slamem_find_mams_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            slamem_mem *mems_dev, uint64_t mems_capacity, uint64_t *block_offsets_dev,
                            void *workspace_dev, uint64_t workspace_bytes, void *stream, uint64_t *total_out);

/* The same batch in MUM mode (option -mum: matchType 2, the mode the reference reserves, slamem.c:35,539, and never built):
 * the -mem rows of a strand block that no other -mem row of the same block contains, in query coordinates or in reference
 * coordinates -- given the complete -mem list, the rows whose string occurs exactly once in the text and once in the scanned
 * strand.  Same arguments, layout and errors as slamem_find_mems_device, rows in the -mem order, every block kept (empty
 * ones too).  mems_capacity must hold the -mem list the filter starts from: when it does not, the call returns
 * SLAMEM_ERR_CAPACITY with *total_out = the -mem count a retry needs; on success *total_out is the MUM count.  The workspace
 * is slamem_find_mums_workspace_bytes() bytes (the -mem workspace and the filter's behind it). */
int slamem_find_mums_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes,
                                     uint64_t mems_capacity, uint64_t *bytes_out);
int slamem_find_mums_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            slamem_mem *mems_dev, uint64_t mems_capacity, uint64_t *block_offsets_dev,
                            void *workspace_dev, uint64_t workspace_bytes, void *stream, uint64_t *total_out);

/* The same batch in SMEM mode (option -smem: matchType 3, the seeds of read mappers): the -mem rows of a
 * strand block whose query interval [q, q+L) no other -mem row of the same block strictly contains -- given the complete
 * -mem list, the rows whose string extends to neither side anywhere in the merged text.  Rows of one interval on different
 * diagonals are its occurrences and are kept together.  max_occ > 0 (option -occ N) drops the intervals that more than max_occ
 * rows of their block share (0: no cap).  Same arguments, layout and errors as slamem_find_mums_device, rows in the -mem
 * order, every block kept (empty ones too), the same capacity rule (SLAMEM_ERR_CAPACITY with *total_out = the -mem count a
 * retry needs).  Every block is decided on the device: one host round trip per batch, as for -mem.  A block whose -mem rows
 * are not in the emission order (query start descending, then length non-increasing) fails the call with SLAMEM_ERR_ARG and
 * a message.  The workspace is slamem_find_smems_workspace_bytes() bytes. */
int slamem_find_smems_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes,
                                      uint64_t mems_capacity, uint64_t *bytes_out);
int slamem_find_smems_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                             uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                             uint32_t max_occ, slamem_mem *mems_dev, uint64_t mems_capacity, uint64_t *block_offsets_dev,
                             void *workspace_dev, uint64_t workspace_bytes, void *stream, uint64_t *total_out);

/* The same batch in chain mode (option -chain: matchType 4): of every strand block's -mem rows, the best
 * collinear chain.  With eq = q + L, ep = p + L and G = max_gap (option -mgap; 0: the default 5000; below 2^31), row j may
 * precede row i iff 0 < q_i - q_j <= G, 0 < p_i - p_j <= G, eq_j < eq_i and ep_j < ep_i; a chain's score is the length of its
 * first row plus min(L_i, eq_i - eq_j, ep_i - ep_j) - |(p_i - q_i) - (p_j - q_j)| for every consecutive pair.  The rows of the
 * block's best chain are kept (ties: DESIGN 4.12), in the -mem order; block_scores_dev (may be NULL) takes a uint32 per
 * strand block, the chain's score, 0 for an empty block.  p is a merged-reference coordinate: a chain may step from one
 * reference record into the next.  Otherwise as slamem_find_smems_device: every block kept (empty ones too), the capacity
 * rule (SLAMEM_ERR_CAPACITY with *total_out = the -mem count a retry needs), one host round trip per batch, a block out of the
 * emission order fails the call with SLAMEM_ERR_ARG.  The workspace is slamem_find_chains_workspace_bytes() bytes. */
int slamem_find_chains_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes,
                                       uint64_t mems_capacity, uint64_t *bytes_out);
int slamem_find_chains_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                              uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                              uint32_t max_gap, slamem_mem *mems_dev, uint64_t mems_capacity, uint64_t *block_offsets_dev,
                              uint32_t *block_scores_dev /* may be NULL */, void *workspace_dev, uint64_t workspace_bytes,
                              void *stream, uint64_t *total_out);

/* The same batch in extension mode (option -ext: matchType 5): every -mem row (p, q, L) of a strand block is
 * extended on its own diagonal, to the left and to the right, through mismatches.  A matching letter scores +1, a mismatch
 * -mismatch_penalty (option -pen; 0: the default 4); a side ends in front of a letter outside either sequence or not one of
 * A,C,G,T, or when the running score has fallen more than xdrop (option -xdrop; SLAMEM_EXT_XDROP_DEFAULT = UINT32_MAX: the
 * default 20; 0 is a value of its own: the side ends at its first mismatch) below its best, and is cut back to the shortest
 * prefix of the best score.  The row becomes (p - extL, q - extL, extL + L + extR); mismatches_dev (may be NULL) takes a
 * uint32 per returned row, the positions inside it whose letters differ, in the order of mems_dev (room for mems_capacity
 * rows).  Of the rows of a block that extend to the same segment only the first is kept; the others keep their order.
 * Otherwise as slamem_find_smems_device: every block kept (empty ones too), the capacity rule (SLAMEM_ERR_CAPACITY with
 * *total_out = the -mem count a retry needs), one host round trip per batch, a block out of the emission order fails the call
 * with SLAMEM_ERR_ARG.  The filter compares the reads with the text planes of the index: an index without them (the COMPACT
 * layout, or one built with the seed sections switched off) is refused with SLAMEM_ERR_ARG and nothing is run.  The workspace
 * is slamem_find_exts_workspace_bytes() bytes. */
#define SLAMEM_EXT_XDROP_DEFAULT 0xFFFFFFFFu
int slamem_find_exts_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes,
                                     uint64_t mems_capacity, uint64_t *bytes_out);
int slamem_find_exts_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands,
                            uint32_t mismatch_penalty, uint32_t xdrop, slamem_mem *mems_dev, uint64_t mems_capacity,
                            uint64_t *block_offsets_dev, uint32_t *mismatches_dev /* may be NULL */, void *workspace_dev,
                            uint64_t workspace_bytes, void *stream, uint64_t *total_out);

/* The same batch in alignment mode (option -aln: matchType 6): per strand block the gapped alignment built on the
 * block's best chain (max_gap as for slamem_find_chains_device).  Consecutive chain rows are joined when the letters between
 * them are A,C,G,T only and their unit-cost edit distance is at most max_edits (option -maxed; SLAMEM_ALN_EDITS_DEFAULT: the
 * default 31; at most 127); a gap that does not close ends a segment.  The block's two outer ends are extended by the X-drop
 * rule of slamem_find_exts_device (mismatch_penalty, xdrop).  segs_dev takes the segments, blocks in the order of -mem, the
 * segments of a block with the query start descending; block_offsets_dev (num_blocks + 1) their offsets per strand block;
 * ops_dev the CIGAR operations of all segments, `length << 4 | op` with BAM's codes (= 7, X 8, I 1, D 2), left to right in the
 * scanned strand; op_offsets_dev (segs_capacity + 1) where each segment's operations start.  mems_capacity is the room for the
 * batch's -mem list, which stays in the workspace.  totals_out[0..2] = -mem rows, segments, operations.  A capacity that is too
 * small gives SLAMEM_ERR_CAPACITY with totals_out holding what a retry needs (after a -mem list that did not fit, [1] and [2]
 * are 0: not known yet).  One host round trip per batch; a block out of the emission order and an index without text planes
 * are refused with SLAMEM_ERR_ARG as for -ext.  The workspace is slamem_find_alns_workspace_bytes() bytes. */
#define SLAMEM_ALN_EDITS_DEFAULT 0xFFFFFFFFu
#define SLAMEM_ALN_EDITS_MAX 127u
/* Gap-affine costs (option -affine) travel in the upper 24 bits of every max_edits word: x per mismatch
 * (1..31), o per gap opened (0..63), e per gap letter (1..31); a gap closes iff its cost is at most o + e * E, which may not
 * exceed SLAMEM_ALN_COST_MAX.  Upper bits of zero: unit cost, as before; SLAMEM_ALN_EDITS_DEFAULT stays unit cost with 31. */
#define SLAMEM_ALN_AFFINE(E, x, o, e) ((uint32_t)(E) | (uint32_t)(x) << 8 | (uint32_t)(o) << 16 | (uint32_t)(e) << 24)
#define SLAMEM_ALN_COST_MAX 512u
/* (include/slamem_aln_word.h decodes and checks such a word, for the library and its front end alike) */
int slamem_find_alns_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t ops_capacity, uint32_t max_edits, uint64_t *bytes_out);
int slamem_find_alns_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap,
                            uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits, uint64_t mems_capacity,
                            slamem_aln *segs_dev, uint64_t segs_capacity, uint64_t *block_offsets_dev, uint32_t *ops_dev,
                            uint64_t ops_capacity, uint64_t *op_offsets_dev, void *workspace_dev, uint64_t workspace_bytes,
                            void *stream, uint64_t *totals_out);

/* Gapped outer ends (option -gext): the forms with end_band beside max_edits.  end_band = Z, 1..31
 * (SLAMEM_ALN_END_BAND_MAX), lets each of a block's two outer ends hold indels of at most Z letters of net diagonal drift: the
 * end is the gapped X-drop attempt of 4.30 when that scores strictly more than the ungapped side, else the ungapped side as
 * before.  It needs gap-affine costs in max_edits (SLAMEM_ALN_AFFINE); 0 is the form without it, byte for byte.  The same
 * holds for slamem_find_maps_*_gext, slamem_find_maps_md_host_gext and slamem_stream_set_end_band (after
 * slamem_stream_set_max_edits, before the first submit).  A workspace is sized with the same end_band as the call it serves. */
#define SLAMEM_ALN_END_BAND_MAX 31u
/* What the last slamem_find_alns_device_gext or slamem_find_maps_device_gext call in workspace_dev did with its outer ends, read
 * from that workspace (the sizing arguments are those of the call; it waits for `stream`): counts_out[0] the ends that went to
 * the gapped attempt (the others were kept inline, fact (c) of DESIGN.md 4.30), counts_out[1] the ends the attempt replaced. */
int slamem_find_alns_end_counts_device(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                       uint64_t ops_capacity, uint32_t max_edits, uint32_t end_band, const void *workspace_dev,
                                       void *stream, uint64_t *counts_out);
int slamem_find_alns_workspace_bytes_gext(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                          uint64_t ops_capacity, uint32_t max_edits, uint32_t end_band, uint64_t *bytes_out);
int slamem_find_alns_device_gext(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                                 uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap,
                                 uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits, uint32_t end_band,
                                 uint64_t mems_capacity, slamem_aln *segs_dev, uint64_t segs_capacity, uint64_t *block_offsets_dev,
                                 uint32_t *ops_dev, uint64_t ops_capacity, uint64_t *op_offsets_dev, void *workspace_dev,
                                 uint64_t workspace_bytes, void *stream, uint64_t *totals_out);
int slamem_find_maps_workspace_bytes_gext(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                          uint64_t ops_capacity, uint32_t max_edits, uint32_t end_band, uint64_t *bytes_out);
int slamem_find_maps_device_gext(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                                 uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap,
                                 uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits, uint32_t end_band,
                                 uint64_t mems_capacity, slamem_aln *segs_dev, uint64_t segs_capacity, uint64_t *read_offsets_dev,
                                 uint32_t *ops_dev, uint64_t ops_capacity, uint64_t *op_offsets_dev, slamem_map *reads_dev,
                                 void *workspace_dev, uint64_t workspace_bytes, void *stream, uint64_t *totals_out);
int slamem_find_alns_host_gext(const slamem_index *idx, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                               uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                               uint32_t max_edits, uint32_t end_band, slamem_aln **segs_out, uint64_t **block_offsets_out,
                               uint32_t **ops_out, uint64_t **op_offsets_out, uint64_t *totals_out);
int slamem_find_maps_host_gext(const slamem_index *idx, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                               uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                               uint32_t max_edits, uint32_t end_band, slamem_aln **segs_out, uint64_t **read_offsets_out,
                               uint32_t **ops_out, uint64_t **op_offsets_out, slamem_map **reads_out, uint64_t *totals_out);
int slamem_find_maps_md_host_gext(const slamem_index *idx, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                                  uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                                  uint32_t max_edits, uint32_t end_band, slamem_aln **segs_out, uint64_t **read_offsets_out,
                                  uint32_t **ops_out, uint64_t **op_offsets_out, slamem_map **reads_out, uint64_t *totals_out,
                                  uint32_t **md_out, uint64_t **md_offsets_out, uint32_t **seg_eq_out, uint32_t **primary_out,
                                  uint64_t *md_total_out);

/* The same batch in mapping mode (option -paf: matchType 7): one mapping per read.  Per read the strand block
 * whose best chain scores highest is the primary one (the forward block on a tie); only that block is aligned, exactly as
 * slamem_find_alns_device aligns it, and the other block gives no segments.  reads_dev takes a slamem_map per read: the strand,
 * the score s1 of the primary chain, the score s2 of the best competing chain (the best chain of the primary block's rows
 * without the primary chain's, or the other block's best chain) and mapq = 60 * (s1 - s2) / s1 in whole numbers.
 * read_offsets_dev (num_queries + 1) takes the segments' offsets per READ.  Segments, operations, capacities, totals_out, errors:
 * as for slamem_find_alns_device; the positions are those of the scanned strand (query_pos on the reverse strand counts in the
 * reverse complement).  The workspace is slamem_find_maps_workspace_bytes() bytes. */
int slamem_find_maps_workspace_bytes(uint32_t num_queries, int both_strands, uint64_t query_bytes, uint64_t mems_capacity,
                                     uint64_t ops_capacity, uint32_t max_edits, uint64_t *bytes_out);
int slamem_find_maps_device(const slamem_index *idx, const void *queries_dev, const uint64_t *offsets_dev,
                            uint32_t num_queries, uint64_t query_bytes, uint32_t min_len, int both_strands, uint32_t max_gap,
                            uint32_t mismatch_penalty, uint32_t xdrop, uint32_t max_edits, uint64_t mems_capacity,
                            slamem_aln *segs_dev, uint64_t segs_capacity, uint64_t *read_offsets_dev, uint32_t *ops_dev,
                            uint64_t ops_capacity, uint64_t *op_offsets_dev, slamem_map *reads_dev, void *workspace_dev,
                            uint64_t workspace_bytes, void *stream, uint64_t *totals_out);

/* ---- (b'+) what SAM needs of a mapped batch (option -sam) ------------------------------------------------------
 * Behind slamem_find_maps_device, over its outputs as they lie on the device: the MD entries of every segment, its letters under
 * `=`, and the primary segment of every read.  Segment s has the entries md_dev[md_offsets_dev[s] .. md_offsets_dev[s + 1]): one
 * uint32 per reference letter under X or D, left to right, `m << 4 | d << 2 | c` -- m the reference letters under `=` since the
 * segment's last entry (or its start; an I changes nothing), d 1 under D, c the text's letter there, A C G T = 0..3 -- and a
 * closing entry `m << 4 | 8`.  (m is below 2^28: a longer run of `=` is outside the contract.)  seg_eq_dev[s] is the letters
 * under `=` of segment s; primary_dev[r] the segment of read r with the largest of them, the first on a tie, as an index into the
 * read's range read_offsets_dev[r] .., 0xFFFFFFFF for a read without segments.
 *   md_capacity   the entries md_dev has room for.  The batch has (letters under X) + (letters under D) + num_segs of them, at
 *                 most (sum of the segments' edits) + num_segs: with that much room the call cannot fail for want of it.  Too
 *                 little: SLAMEM_ERR_CAPACITY, *md_total the need, and no word at or behind md_dev[md_capacity] is written.
 *   md_offsets_dev  num_segs + 1 entries.  num_segs == 0 is valid: md_offsets_dev[0] = 0, every primary 0xFFFFFFFF.
 * Everything runs on `stream`; the call ends with one copy of the total to the host and waits for it.  The letters come from the
 * text planes of the index: one without them (the COMPACT layout) is refused with SLAMEM_ERR_ARG and nothing is run.  The
 * workspace is slamem_maps_md_workspace_bytes() bytes.  slamem_find_maps_md_host: slamem_find_maps_host plus the four arrays
 * (malloc()ed, released with slamem_host_free) and their number of entries. */
int slamem_maps_md_workspace_bytes(uint64_t num_segs, uint32_t num_queries, uint64_t *bytes_out);
int slamem_maps_md_device(const slamem_index *idx, const slamem_aln *segs_dev, uint64_t num_segs, const uint64_t *read_offsets_dev,
                          uint32_t num_queries, const uint32_t *ops_dev, const uint64_t *op_offsets_dev, uint32_t *md_dev,
                          uint64_t md_capacity, uint64_t *md_offsets_dev /* num_segs + 1 */, uint32_t *seg_eq_dev,
                          uint32_t *primary_dev, void *workspace_dev, uint64_t workspace_bytes, void *stream, uint64_t *md_total);
int slamem_find_maps_md_host(const slamem_index *idx, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                             uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                             uint32_t max_edits, slamem_aln **segs_out, uint64_t **read_offsets_out, uint32_t **ops_out,
                             uint64_t **op_offsets_out, slamem_map **reads_out, uint64_t *totals_out, uint32_t **md_out,
                             uint64_t **md_offsets_out, uint32_t **seg_eq_out, uint32_t **primary_out, uint64_t *md_total_out);

/* ---- (b'') per-base pileup of the read mappings (option -pile: matchType 8) ----------------------------------
 * What a user does with -paf's mappings: pile them onto the reference.  With n the merged text's length the table has n rows of
 * six uint32 counters in the order A, C, G, T, D, I.  A read contributes iff its record has strand != 0 and mapq >= min_mapq;
 * then each of its segments is walked once, left to right, p from ref_pos and q from query_pos in the scanned strand: an = or X
 * of k counts the scanned strand's letter (upper-cased; a letter that is none of A,C,G,T is counted nowhere) in its column at
 * rows p .. p+k-1; a D of k counts in column D of rows p .. p+k-1; an I of k counts ONCE, in column I of row p (the insertion
 * stands in front of reference letter p; at p == n it is dropped).  Depth at a row is A+C+G+T+D.  The table is the sum over all
 * batches added since creation or the last reset: addition commutes, so it does not depend on how the reads were split into
 * batches, on their order, on the stream or on the GPU.  Counters are 32 bits wide: a true depth of 2^31 or more at one row is
 * outside the contract.
 *
 *   slamem_pileup_create   the accumulator lives on the index's device and takes 28 bytes per text letter (a difference array
 *                          for the = runs, 4 bytes, and the table of what differs from the text, 24).  Too little free HBM:
 *                          SLAMEM_ERR_NOMEM with the numbers in the message.  It reads the text planes of the index: an index
 *                          without them (the COMPACT layout) is refused with SLAMEM_ERR_ARG.  The index must outlive it.
 *   slamem_pileup_reset    all counters to 0 (waits for the device first)
 *   slamem_pileup_add_device  takes the outputs of slamem_find_maps_device as they are, with the batch's queries and offsets.
 *                          Asynchronous on `stream`; nothing is validated that would need a read-back (every write is checked
 *                          against n on the device); min_mapq above 60: SLAMEM_ERR_ARG.  Adds from several streams and threads
 *                          into one accumulator are safe: every update is an atomic add.
 *   slamem_pileup_counts_device  rows [first, first + count) as count x 6 uint32, asynchronous on `stream`, ordered behind the
 *                          adds of that stream.  The accumulator is not modified: more batches may be added and the table read
 *                          again.  Two read-outs of one accumulator must not run at the same time (they share a small scratch).
 *                          A range outside [0, n]: SLAMEM_ERR_ARG.
 *   slamem_pileup_counts_host  the same into host memory; waits for the device first, so it sees the adds of every stream. */
typedef struct slamem_pileup slamem_pileup;
int slamem_pileup_create(const slamem_index *idx, slamem_pileup **out);
int slamem_pileup_free(slamem_pileup *pile);
int slamem_pileup_reset(slamem_pileup *pile);
int slamem_pileup_add_device(slamem_pileup *pile, const void *queries_dev, const uint64_t *offsets_dev, uint32_t num_queries,
                             const slamem_aln *segs_dev, const uint64_t *read_offsets_dev, const uint32_t *ops_dev,
                             const uint64_t *op_offsets_dev, const slamem_map *reads_dev, uint32_t min_mapq, void *stream);
int slamem_pileup_counts_device(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t *out_dev, void *stream);
int slamem_pileup_counts_host(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t *out);

/* ---- (b'' 2) base quality: the low-quality mask of a batch (option -bq) ----------------------------------------
 * A batch may come with a low-quality mask: a bit array over its letter buffer, indexed as the letters are.  Bit j (bit j % 64 of
 * word j / 64 of a uint64 array of (total_letters + 63) / 64 words) belongs to queries[j], so bit offsets[r] + i belongs to letter
 * i of read r AS GIVEN; reads share words.  With a mask, a letter whose bit is set counts NOWHERE under = or X: the row gets nothing
 * from this read and its depth does not rise.  On strand 2 the scanned strand's letter q is the given letter len - 1 - q and has
 * that letter's bit.  D rows, I operations and the indel events are as without a mask (samtools mpileup -Q does the same).  A mask
 * without a set bit, or NULL, gives bit for bit what slamem_pileup_add_device gives; addition still commutes.
 *
 * The mask is made from quality bytes by one rule: letter j is low iff max(0, qual[j] - phred_offset) < min_bq.  min_bq is 0 to
 * 93 (0: nothing is low), phred_offset 0 to 126 (33 for FASTQ as it is written today); anything else: SLAMEM_ERR_ARG.  The unused
 * bits of the last word are 0.
 *   slamem_pack_lowq_device  quality bytes in device memory -> mask_out_dev, asynchronous on `stream`
 *   slamem_pack_lowq       the same on the host with `threads` threads: what a front end puts in front of
 *                          slamem_stream_submit_masked, so that the link carries an eighth of a byte per letter, not one
 *   slamem_pileup_add_masked_device  slamem_pileup_add_device with the batch's mask in device memory; no word at or behind
 *                          (offsets[num_queries] + 63) / 64 is read, and none that holds no bit of a read.  NULL: the unmasked
 *                          add.  slamem_pileup_add_device stays as it is. */
int slamem_pack_lowq_device(const void *quals_dev, uint64_t total_letters, uint32_t min_bq, uint32_t phred_offset,
                            uint64_t *mask_out_dev, void *stream);
int slamem_pack_lowq(const char *quals, uint64_t total_letters, uint32_t min_bq, uint32_t phred_offset, uint64_t *mask_out,
                     int threads);
int slamem_pileup_add_masked_device(slamem_pileup *pile, const void *queries_dev, const uint64_t *offsets_dev, uint32_t num_queries,
                                    const slamem_aln *segs_dev, const uint64_t *read_offsets_dev, const uint32_t *ops_dev,
                                    const uint64_t *op_offsets_dev, const slamem_map *reads_dev, uint32_t min_mapq,
                                    const uint64_t *lowq_dev, void *stream);

/* ---- (b''') the sparse read-out of the pileup (option -sites) ------------------------------------------------
 * The rows of [first, first + count) that a rule selects, compacted on the device in ascending position.  cnt[p] is row p as
 * slamem_pileup_counts_* gives it, L(p) the text's letter at p in upper case, d(p) = A+C+G+T+D (a 64-bit sum).
 *   SLAMEM_SITES_NONZERO (0)  row p is selected iff one of its six counters is not 0; bit k of its allele mask is set iff
 *                          cnt[p][k] != 0 (k in the order A C G T D I).  The thresholds and the letter play no part.
 *   SLAMEM_SITES_VARIANT (1)  row p is selected iff L(p) is one of A,C,G,T, d(p) >= min_depth and its mask is not 0, where bit
 *                          k (k not the column of L(p)) is set iff cnt[p][k] > 0 and 100 * cnt[p][k] >= min_pct * d(p), the
 *                          products formed in 64 bits.  min_depth is 1 to 2^31 - 1, min_pct 0 to 100.
 * The result is three arrays of `total` entries: pos (uint64), counts (uint32 x 6) and alleles (uint8, the mask).  It depends on
 * the table alone, not on how the table came to be.  VCF is not written from it: the accumulator knows how many reads insert in
 * front of a row, not what they insert, and it counts a deletion per row, not per event.
 *
 *   slamem_pileup_sites_device  asynchronous on `stream` up to its one host round trip, which brings the number of selected
 *                          rows to *total_out (a host pointer).  More than `capacity`: SLAMEM_ERR_CAPACITY with *total_out
 *                          holding the need; the first `capacity` rows are written and nothing beyond them.  A range outside
 *                          [0, n], a mode above 1, min_pct above 100, and in mode 1 a min_depth of 0 or of 2^31 and more:
 *                          SLAMEM_ERR_ARG.  It shares the read-outs' scratch: two read-outs of one accumulator must not run at
 *                          the same time.  The accumulator is not modified.
 *   slamem_pileup_sites_host  the same into host memory; waits for the device first, so it sees the adds of every stream.
 *   slamem_pileup_add_counts_device  cnt[first + i][k] += rows[i][k] for a table of count x 6 uint32, asynchronous on `stream`:
 *                          atomic adds, so it commutes with the adds of other streams.  The rows of slamem_pileup_counts_* of
 *                          another accumulator make this one's read-out the sum of both tables.
 *   slamem_pileup_add_counts_host  the same from host memory; returns when the table is added. */
#define SLAMEM_SITES_NONZERO 0u
#define SLAMEM_SITES_VARIANT 1u
int slamem_pileup_sites_device(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t mode, uint32_t min_depth,
                               uint32_t min_pct, uint64_t capacity, uint64_t *pos_dev, uint32_t *counts_dev, uint8_t *alleles_dev,
                               uint64_t *total_out, void *stream);
int slamem_pileup_sites_host(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t mode, uint32_t min_depth,
                             uint32_t min_pct, uint64_t capacity, uint64_t *pos, uint32_t *counts, uint8_t *alleles,
                             uint64_t *total_out);
int slamem_pileup_add_counts_device(slamem_pileup *pile, uint64_t first, uint64_t count, const uint32_t *rows_dev, void *stream);
int slamem_pileup_add_counts_host(slamem_pileup *pile, uint64_t first, uint64_t count, const uint32_t *rows);

/* ---- (b'''') the indel events of the pileup (option -vcf) -----------------------------------------------------
 * What the table above does not hold: WHICH letters the reads insert, and a deletion as one event.  With events enabled every
 * slamem_pileup_add_device also records, for each contributing read, its I operations (an insertion of S = the k upper-cased
 * letters of the scanned strand, in front of row p) and its D operations (a deletion of rows [p, p + k)), each left-normalised
 * against the text: a deletion moves left while the letter in front of it equals its last letter, an insertion while the letter
 * in front of it equals the last letter of S (which then rotates); both stop at row 0 and at a letter that is none of A,C,G,T, so
 * no event leaves its record.  The table maps (pos, kind, len, S) to fwd and rev, the observations from reads of strand 1 and of
 * strand 2 (uint32, modulo 2^32), summed over everything added since slamem_pileup_enable_events or the last reset, whatever the
 * batches, their order, the streams and the GPUs.  The columns A C G T D I of the table above stay as aligned, not normalised.
 * Observations that are counted and not stored -- skipped[0]: an insertion of more than 31 letters; skipped[1]: an observation
 * the hash table had no room for (more slots help); skipped[2]: an insertion at row n or with a letter that is none of A,C,G,T,
 * a deletion of more than 127 rows, beyond row n or over a row that is none of A,C,G,T (none should occur on the engine's own
 * mappings).
 *
 * slamem_event: kind 0 a deletion of len rows from pos, kind 1 an insertion of len letters in front of pos; letters: the
 * inserted letters two bits each (A 0, C 1, G 2, T 3), letter i at bits 2 * (len - 1 - i), 0 for a deletion.
 *
 *   slamem_pileup_enable_events  allocates the hash table of `slots` slots (a power of two of at least 64; 0: the smallest power
 *                          of two that is at least max(65536, n / 16)) of 24 bytes and as much again for the read-out's sort.  Too
 *                          little free HBM: SLAMEM_ERR_NOMEM with the numbers; enabled already, or a bad number of slots:
 *                          SLAMEM_ERR_ARG.  Waits for the device.  slamem_pileup_reset also clears the events and skipped.
 *   slamem_pileup_events_device  the events with first <= pos < first + count and fwd + rev >= min_count (>= 1), ascending in
 *                          (pos, kind, len, S), S letter by letter with A < C < G < T, and the three skipped counters (host
 *                          pointers, as total_out).  Asynchronous on `stream` but for one host round trip.  More than `capacity`:
 *                          SLAMEM_ERR_CAPACITY with the need in *total_out and the first `capacity` events written; capacity 0
 *                          with a null buffer asks for the count alone.  Events not enabled, a range outside [0, n],
 *                          min_count 0: SLAMEM_ERR_ARG.  The table is not modified.  Two read-outs of one accumulator must not
 *                          run at the same time, and none beside an add (they share scratch; an add may be half-way in a slot).
 *   slamem_pileup_events_host  the same into host memory; waits for the device first.
 *   slamem_pileup_add_events_device  every given event is validated as an observation is, normalised (a canonical event stays as
 *                          it is) and added with its fwd and rev: the merge of another accumulator's events.  Asynchronous.
 *   slamem_pileup_add_events_host  the same from host memory; returns when the events are added.
 *   slamem_pileup_rows_at_device  the rows of slamem_pileup_counts_* at m listed positions (m x 6 uint32), asynchronous; a position
 *                          at or beyond n gives a row of zeros.  Shares the read-outs' scratch.  Needs no events.
 *   slamem_pileup_rows_at_host  the same from and into host memory; a position at or beyond n: SLAMEM_ERR_ARG. */
typedef struct {
    uint64_t pos;
    uint64_t letters;
    uint32_t fwd, rev;
    uint8_t kind, len;
    uint8_t pad[6]; /* 0 */
} slamem_event;
int slamem_pileup_enable_events(slamem_pileup *pile, uint64_t slots);
int slamem_pileup_events_device(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t min_count, uint64_t capacity,
                                slamem_event *events_dev, uint64_t *skipped_out /* 3 */, uint64_t *total_out, void *stream);
int slamem_pileup_events_host(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t min_count, uint64_t capacity,
                              slamem_event *events, uint64_t *skipped_out /* 3 */, uint64_t *total_out);
int slamem_pileup_add_events_device(slamem_pileup *pile, const slamem_event *events_dev, uint64_t m, void *stream);
int slamem_pileup_add_events_host(slamem_pileup *pile, const slamem_event *events, uint64_t m);
int slamem_pileup_rows_at_device(slamem_pileup *pile, const uint64_t *pos_dev, uint64_t m, uint32_t *out_dev, void *stream);
int slamem_pileup_rows_at_host(slamem_pileup *pile, const uint64_t *pos, uint64_t m, uint32_t *out);

/* ---- (b''''') the consensus sequence of the pileup (option -cons) --------------------------------------------
 * The text with the majority alleles applied, one byte per emitted letter.  cnt[p], L(p) and d(p) as above; ACGT(p): L(p) is one
 * of A,C,G,T; E: the events as slamem_pileup_events_* reads them out with min_count 1, in its order (empty when events are not
 * enabled); obs = fwd + rev in 64 bits.  The anchor row of an event at pos is a = pos - 1 if pos >= 1 and ACGT(pos - 1), else
 * a = pos.  An event is applied iff ACGT(a), d(a) >= min_depth and 2 * obs > d(a).  Row p emits, in this order:
 *   1. of the applied insertions with pos == p the one with the largest obs (a tie: the first in E's order): its len letters in
 *      upper case -- also when rule 2 drops the row;
 *   2. nothing more if an applied deletion covers p (pos <= p < pos + len);
 *   3. else N if not ACGT(p);
 *   4. else L(p) in lower case if d(p) < min_depth or A+C+G+T == 0 (the row is uncalled, the text is kept);
 *   5. else in upper case the letter with the largest of the counters A,C,G,T; a tie: L(p) if its counter is among the largest,
 *      else the first of the tied in the order A,C,G,T.
 * The consensus of rows [first, first + count) is the concatenation of their emissions; a row's emission does not depend on the
 * range (the anchor of an event at `first` may be row first - 1), so every range's output is a slice of the whole text's.  For
 * m bounds in [first, first + count], offs[j] is the number of bytes that rows [first, bounds[j]) emit: an insertion in front of
 * row bounds[j] lies behind offs[j].  stats: rows uncalled (rule 4), rows whose called letter differs from L(p) (rule 5), rows
 * deleted (rule 2), insertions emitted, letters inserted.
 *
 *   slamem_pileup_consensus_device  asynchronous on `stream` up to the host round trip that brings the number of bytes to
 *                          *total_out and the statistics to stats_out (host pointers); with events enabled the events' read-out
 *                          in front of it makes its own (the sort needs the number of events on the host).  More than `capacity`
 *                          bytes: SLAMEM_ERR_CAPACITY with the need in *total_out; the first `capacity` bytes are written and
 *                          nothing beyond them; capacity 0 with a null buffer asks for the size.  offs is complete either way.
 *                          bounds_dev may be null with m = 0; a bound outside the range gets UINT64_MAX.  A range outside [0, n],
 *                          min_depth of 0 or of 2^31 and more: SLAMEM_ERR_ARG.  The accumulator and the events are not
 *                          modified.  It shares the read-outs' scratch and keeps a byte per text letter of its own from the first
 *                          call to slamem_pileup_free: two read-outs of one accumulator must not run at the same time, and none
 *                          beside an add.
 *   slamem_pileup_consensus_host  the same from and into host memory; waits for the device first.  A bound outside the range:
 *                          SLAMEM_ERR_ARG. */
int slamem_pileup_consensus_device(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t min_depth, uint64_t capacity,
                                   uint8_t *out_dev, const uint64_t *bounds_dev, uint64_t m, uint64_t *offs_dev,
                                   uint64_t *stats_out /* 5 */, uint64_t *total_out, void *stream);
int slamem_pileup_consensus_host(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t min_depth, uint64_t capacity,
                                 uint8_t *out, const uint64_t *bounds, uint64_t m, uint64_t *offs, uint64_t *stats_out /* 5 */,
                                 uint64_t *total_out);

/* ---- (b'''''') the depth of coverage as runs (option -depth) -------------------------------------------------
 * d(p) as above, the 64-bit sum of row p's first five counters as slamem_pileup_counts_* gives them.  Levels t_1 < ... < t_k
 * (k from 0 to 16, each at least 1, strictly ascending; a host array): the value of a row is v(p) = d(p) when k == 0, else the
 * number of i with t_i <= d(p), 0 to k.  Row p of the range [first, first + count) is a head iff p == first or v(p) != v(p - 1).
 * The result is the heads in ascending p as records {pos, value}: run i spans [pos[i], pos[i + 1]), the last one ends at
 * first + count, an empty range has no run, runs of depth 0 are runs like the others -- the runs tile the range.  Head-ness
 * depends on v(p) and v(p - 1) alone, so the runs of any range are the whole text's runs clipped to it.  For m bounds, non-
 * decreasing in [first, first + count], cum[j] is the pair (sum of d(p), number of p with d(p) >= min_depth) over rows
 * first <= p < bounds[j]; a range's cum differs from the whole text's by the constant pair at `first`.
 *
 *   slamem_pileup_depth_runs_device  asynchronous on `stream` up to the one host round trip that brings the number of runs to
 *                          *total_out (a host pointer).  More than `capacity` runs: SLAMEM_ERR_CAPACITY with the need in
 *                          *total_out; the first `capacity` runs are written and nothing beyond them; capacity 0 with a null
 *                          buffer asks for the size.  cum is complete either way.  bounds_dev may be null with m = 0; bounds
 *                          outside the range or descending get unspecified cum entries, and nothing outside the buffers is
 *                          accessed.  SLAMEM_ERR_ARG: a range outside [0, n], more than 16 levels, a level of 0 or levels that do
 *                          not ascend strictly, min_depth of 0 or of 2^31 and more, a null pile or total_out.  The accumulator is
 *                          not modified.  It shares the read-outs' tile sums and keeps three numbers per tile of its own from the
 *                          first call to slamem_pileup_free: two read-outs of one accumulator must not run at the same time, and
 *                          none beside an add.
 *   slamem_pileup_depth_runs_host  the same from and into host memory; waits for the device first.  A bound outside the range or
 *                          smaller than the bound in front of it: SLAMEM_ERR_ARG. */
typedef struct {
    uint64_t pos;   /* the run's first row */
    uint64_t value; /* d of its rows, or with levels the number of levels they reach */
} slamem_depth_run;

int slamem_pileup_depth_runs_device(slamem_pileup *pile, uint64_t first, uint64_t count, const uint32_t *levels /* host */,
                                    uint32_t num_levels, uint32_t min_depth, uint64_t capacity, slamem_depth_run *runs_dev,
                                    const uint64_t *bounds_dev, uint64_t m, uint64_t *cum_dev /* 2 m */, uint64_t *total_out,
                                    void *stream);
int slamem_pileup_depth_runs_host(slamem_pileup *pile, uint64_t first, uint64_t count, const uint32_t *levels, uint32_t num_levels,
                                  uint32_t min_depth, uint64_t capacity, slamem_depth_run *runs, const uint64_t *bounds, uint64_t m,
                                  uint64_t *cum /* 2 m */, uint64_t *total_out);

/* ---- (b''''''') duplicate reads counted once (option -dedup) -----------------------------------------------------
 * A read is a candidate iff it would contribute to the pileup: strand != 0, mapq >= min_mapq, at least one segment.  Its key is
 * (strand, u), u the unclipped 5' position in merged-text coordinates (signed; len the read's length):
 *   strand 1   L the segment with the smallest query_pos:             u = ref_pos(L) - query_pos(L)
 *   strand 2   R the segment with the largest query_pos + query_len:  u = ref_pos(R) + ref_len(R) + (len - query_pos(R) - query_len(R))
 * Every dedup add of an accumulator gets a sequence number when it is enqueued; a read's rank is seq << 32 | its index in the
 * batch.  A candidate is a duplicate iff another candidate with the same key has a smaller rank, and a duplicate is not piled: no
 * counter, no diff, no indel event.  So one read per key is piled, the first in enqueue order and then in batch order -- with one
 * stream, file order.  ADDITION WITH DEDUP DOES NOT COMMUTE ACROSS ADDS: the table of the counters is the same sum whatever the
 * order, but which reads it is the sum of depends on the order the adds were enqueued in.
 * The keys live in an open-addressing table in HBM beside the accumulator (16 bytes a slot, linear probing with a probe limit); a
 * candidate that finds no slot within the limit is kept and counted as "no room".
 *   slamem_pileup_enable_dedup  allocates the table of `slots` slots (a power of two from 64 to 2^32; 0: the smallest power of two
 *                          that is at least 65,536 and a quarter of n; anything else SLAMEM_ERR_ARG).  Too little HBM:
 *                          SLAMEM_ERR_NOMEM with the numbers.  A second call: SLAMEM_ERR_ARG.  Waits for the device.
 *                          slamem_pileup_reset also clears the table, the counters and the sequence number; slamem_pileup_free
 *                          releases them.
 *   slamem_pileup_add_dedup_device  slamem_pileup_add_masked_device (lowq_dev may be NULL) behind the filter: reads_keep_dev takes
 *                          num_queries records, the read records with strand 0 where the read is a duplicate, and is what the add
 *                          kernels read -- it must stay until they are through; dup_out_dev (may be NULL) a byte per read: 0 kept
 *                          or no candidate, 1 duplicate, 2 no room (kept).  reads_dev is left as it is.  Without
 *                          slamem_pileup_enable_dedup: SLAMEM_ERR_ARG.  The filter's kernels of two such adds on one accumulator
 *                          never overlap on the device, whatever streams they are enqueued on (a host mutex, an event); the add
 *                          kernels behind them overlap freely.
 *   slamem_pileup_dedup_stats  candidates, duplicates, candidates without room, slots newly claimed (= candidates kept with a
 *                          slot: out[0] = out[1] + out[2] + out[3]), summed since the table was enabled or reset.  Waits for the
 *                          device.
 * slamem_pileup_add_device and slamem_pileup_add_masked_device on such an accumulator add every read as before, and
 * slamem_pileup_add_counts_* and slamem_pileup_add_events_* bypass the filter: what they add are counts, not reads.
 *   slamem_stream_set_dedup  on != 0: the download stage of a stream of match type 8 adds every batch with the filter; before the
 *                          first submit, behind slamem_stream_set_pileup with an accumulator whose filter is enabled
 *                          (SLAMEM_ERR_ARG otherwise).  slamem_stream_maps still gives the read records as the search wrote them.
 *   slamem_stream_dups     the flags (a byte per read) of the batch slamem_stream_next returned last, in the stream's pinned
 *                          memory, valid as long as that batch.  SLAMEM_ERR_ARG on a stream whose filter is not switched on. */
int slamem_pileup_enable_dedup(slamem_pileup *pile, uint64_t slots);
int slamem_pileup_add_dedup_device(slamem_pileup *pile, const void *queries_dev, const uint64_t *offsets_dev, uint32_t num_queries,
                                   const slamem_aln *segs_dev, const uint64_t *read_offsets_dev, const uint32_t *ops_dev,
                                   const uint64_t *op_offsets_dev, const slamem_map *reads_dev, uint32_t min_mapq,
                                   const uint64_t *lowq_dev, slamem_map *reads_keep_dev, uint8_t *dup_out_dev, void *stream);
int slamem_pileup_dedup_stats(slamem_pileup *pile, uint64_t out[4]);

/* ---- (b'''''''') diploid genotypes of the pileup (option -gt) ----------------------------------------------------
 * A likelihood-based call per row and per indel event, all in unsigned 64-bit integers, scores in milli-Phred.  The parameters:
 * ploidy 1 or 2; match_cost M, het_cost H, err_cost E: what one observed letter costs a genotype that is homozygous for it,
 * heterozygous with it, or does not hold it (H and E from 1, M from 0, none above 2^20; slamem_gt_costs gives the three for a
 * constant error rate of Phred q, q = 20: 44, 3039, 24771); het_prior hp (0 to 2^20): the cost per non-reference allele of a
 * genotype; min_depth as for -sites (1 to 2^31 - 1); min_qual in Phred, 0 to 999.
 *   SNV rows   c[0..3] the A C G T columns of row p, r the column of L(p), d(p) = A+C+G+T+D.  Ploidy 2: the ten genotypes (j, k),
 *              j <= k, at index g = k (k + 1) / 2 + j (AA AC CC AG CG GG AT CT GT TT); L_g = sum_i c[i] w(i, g), w = M when
 *              i == j == k, H when j != k and i is one of them, else E.  Ploidy 1: the four genotypes i, L_i = c[i] M + (the
 *              others) E.  S_g = L_g + hp * (distinct letters of g that are not r).  The best genotype has the smallest S; on a
 *              tie the homozygous-reference one wins, then the smallest g.  qual = S_rr - S_best, gq = the smallest S_g - S_best
 *              over g != best, pl[g] = L_g - min L; each saturates at 2^32 - 1 when stored.  Row p is selected iff L(p) is one of
 *              A,C,G,T, d(p) >= min_depth, the best genotype is not rr and qual >= 1000 * min_qual.
 *   events     ao = fwd + rev, d the depth of the anchor row, ro = d > ao ? d - ao : 0; L_00 = ro M + ao E, L_01 = (ro + ao) H
 *              (ploidy 2 only), L_11 = ao M + ro E, priors 0, hp, hp; best, qual, gq and pl[0..2] (pl[0..1] at ploidy 1) as
 *              above; called iff d >= min_depth, the best genotype is not 00 and qual >= 1000 * min_qual.  Every event stands
 *              alone against everything else at its anchor: two events of one anchor are not made one multi-allelic call.
 * slamem_genotype: a <= b are letter columns (SNV) or allele numbers 0 / 1 (event), both the one allele at ploidy 1; ref is r (0
 * for an event); unused pl entries and the padding are 0.
 *   slamem_gt_costs        host code: out[0..2] = M, H, E of q in 1 .. 93 with e = 10^(-q/10): round(-10000 log10(1 - e)),
 *                          round(-10000 log10((1 - e) / 2 + e / 6)), round(-10000 log10(e / 3)); another q: SLAMEM_ERR_ARG.
 *   slamem_pileup_genotypes_device  the selected rows of [first, first + count) in ascending position: pos (uint64), counts
 *                          (uint32 x 6) and gts, with the capacity contract of slamem_pileup_sites_device: asynchronous up to the
 *                          one host round trip that brings the number of selected rows to *total_out; more than `capacity`:
 *                          SLAMEM_ERR_CAPACITY with the need there, the first `capacity` rows written and nothing beyond them.
 *                          SLAMEM_ERR_ARG: a range outside [0, n] or parameters outside the ranges above.  It shares the
 *                          read-outs' scratch: two read-outs of one accumulator must not run at the same time.
 *   slamem_pileup_genotypes_host  the same into host memory; waits for the device first.
 *   slamem_pileup_genotype_events_device  m events (as slamem_pileup_events_* gives them) and the m x 6 rows of their anchors (as
 *                          slamem_pileup_rows_at_device gives them), both in device memory: a slamem_genotype and a `called`
 *                          byte (0 / 1) per event; asynchronous on `stream`.
 *   slamem_pileup_genotype_events_host  the same from and into host memory, with the anchors as m positions: their rows are
 *                          read on the device.  An anchor at or beyond n: SLAMEM_ERR_ARG. */
typedef struct {
    uint32_t ploidy;     /* 1 or 2 */
    uint32_t match_cost; /* M */
    uint32_t het_cost;   /* H */
    uint32_t err_cost;   /* E */
    uint32_t het_prior;  /* hp */
    uint32_t min_depth;
    uint32_t min_qual;   /* Phred */
} slamem_gt_params;
typedef struct {
    uint32_t qual, gq;
    uint8_t a, b, ploidy, ref;
    uint32_t pl[10];
    uint8_t pad[4];
} slamem_genotype; /* 56 bytes */
int slamem_gt_costs(uint32_t q, uint32_t out[3]);
int slamem_pileup_genotypes_device(slamem_pileup *pile, uint64_t first, uint64_t count, const slamem_gt_params *params,
                                   uint64_t capacity, uint64_t *pos_dev, uint32_t *counts_dev, slamem_genotype *gts_dev,
                                   uint64_t *total_out, void *stream);
int slamem_pileup_genotypes_host(slamem_pileup *pile, uint64_t first, uint64_t count, const slamem_gt_params *params,
                                 uint64_t capacity, uint64_t *pos, uint32_t *counts, slamem_genotype *gts, uint64_t *total_out);
int slamem_pileup_genotype_events_device(slamem_pileup *pile, const slamem_event *events_dev, const uint32_t *anchor_rows_dev,
                                         uint64_t m, const slamem_gt_params *params, slamem_genotype *gts_dev, uint8_t *called_dev,
                                         void *stream);
int slamem_pileup_genotype_events_host(slamem_pileup *pile, const slamem_event *events, const uint64_t *anchors, uint64_t m,
                                       const slamem_gt_params *params, slamem_genotype *gts, uint8_t *called);

/* ---- (b''''''''') strand counts of the pileup (option -sb) -------------------------------------------------------
 * An accumulator with strand counts owns a second one of the same layout, the forward accumulator, which receives exactly the
 * contributions of the reads of strand 1 -- in the same kernels, which walk every read once and issue the atomics of such a read
 * on both.  It is an ordinary accumulator without events and without a duplicate filter: every read-out (counts, rows_at, sites,
 * genotypes, consensus, depth_runs) works on it, and the reverse strand's rows are the owner's minus its.  28 more bytes per
 * text letter.
 *   slamem_pileup_enable_strands  allocates the forward accumulator.  Only on an empty accumulator -- just created, or reset: after
 *                          any add SLAMEM_ERR_ARG; a second call is a no-op.  Too little free device memory: SLAMEM_ERR_NOMEM.
 *                          slamem_pileup_reset of the owner clears both, slamem_pileup_free frees both.
 *   slamem_pileup_forward  the forward accumulator, borrowed: valid until the owner is freed.  Not enabled: SLAMEM_ERR_ARG.
 * The borrowed handle refuses slamem_pileup_add_device, _add_masked_device, _add_dedup_device, _add_events_*, _enable_events,
 * _enable_dedup, _enable_strands, slamem_stream_set_pileup and slamem_pileup_free with SLAMEM_ERR_ARG; slamem_pileup_add_counts_*
 * on it is allowed (the tables of several GPUs are added up that way).
 *   slamem_fisher_strand   host code: FS, the Phred-scaled two-sided Fisher exact test of the table t = (reference forward,
 *                          reference reverse, alternative forward, alternative reverse), in doubles (slamem_fisher.h has the
 *                          steps); 0 for an empty table or NULL.
 *   slamem_fisher_strand_table  the table after the normalisation of its first step (cells of a sum above 400 scaled to 200). */
int slamem_pileup_enable_strands(slamem_pileup *pile);
int slamem_pileup_forward(slamem_pileup *pile, slamem_pileup **out);
double slamem_fisher_strand(const uint32_t t[4]);
void slamem_fisher_strand_table(const uint32_t t[4], uint32_t out[4]);

/* ---- (b'''''''''') quality sums of the pileup and the weighted genotypes -----------------------------------------
 * An accumulator with quality sums owns a second one of the same layout, the quality accumulator Q.  A letter's quality is
 * qv(b) = 0 when its byte b is below the Phred offset, else min(b - offset, 93); the quality of letter x of the scanned strand of a
 * strand-2 read is the byte at len - 1 - x.  Every read that contributes to the pileup of an add contributes to Q (the same
 * min_mapq, low-quality mask and duplicate decision): wherever the pileup's walk adds 1 to column A, C, G or T of a row, Q gets qv
 * of that letter in the same column of the same row.  D and I add nothing: those two columns of Q stay 0.  So
 * Q[p][c] <= 93 * counts[p][c], and with every quality equal to q, Q = q * counts on the four letter columns.  Sums are taken
 * modulo 2^32: a depth below 2^25 at a row is inside the contract.  28 more bytes per text letter.
 *   slamem_pileup_enable_quals  allocates Q.  Only on an empty accumulator -- just created, or reset: after any add
 *                          SLAMEM_ERR_ARG; a second call is a no-op.  Too little free device memory: SLAMEM_ERR_NOMEM.
 *                          slamem_pileup_reset of the owner clears both, slamem_pileup_free frees both.  It combines with
 *                          _enable_strands, _enable_events and _enable_dedup in any order.
 *   slamem_pileup_quality  Q, borrowed: valid until the owner is freed.  Not enabled: SLAMEM_ERR_ARG.  The read-outs with a
 *                          meaning on it are slamem_pileup_counts_*, _rows_at_* and _add_counts_* (the tables of several GPUs are
 *                          added up that way); it refuses what the forward accumulator refuses, and _enable_quals.
 *   slamem_pileup_add_quals_device  the add of an accumulator with quality sums, the superset of slamem_pileup_add_device,
 *                          _add_masked_device and _add_dedup_device: lowq_dev may be NULL (no mask); quals_dev holds a byte per
 *                          letter, indexed as queries_dev is; dedup != 0 sends the batch through the duplicate filter (which must be
 *                          enabled) and needs reads_keep_dev, dup_out_dev may be NULL.  The quality pass is a second pair of kernels
 *                          behind the pile kernels of the same add on `stream`.  On an accumulator with quality sums the three
 *                          other add entries are refused with SLAMEM_ERR_ARG -- Q would fall behind the counts; on one without,
 *                          this entry is.
 *   slamem_pileup_genotypes_weighted_device / _host  slamem_pileup_genotypes_* with one change and one more output: a letter i that
 *                          a genotype does not hold costs c[i] * err_cost + 1000 * Q[i] in the place of c[i] * err_cost, and
 *                          qsums gets the A C G T columns of Q's row, four uint32 per selected row (room for `capacity` rows).
 *                          Best genotype, tie rule, qual, gq, pl, selection, saturation and the capacity contract are those of
 *                          slamem_pileup_genotypes_*.  1000 * 2^32 < 2^42 per letter keeps every sum below 2^56.  -wq's costs are
 *                          match_cost 0, het_cost 3010, err_cost 4771 (round(10000 log10 2) and round(10000 log10 3)): a
 *                          miscalled letter of quality q costs 1000 q + 4771 = round(-10000 log10(e / 3)).  With Q all zero the
 *                          read-out equals slamem_pileup_genotypes_* byte for byte; with every letter at quality q it equals it
 *                          with err_cost + 1000 q.  Not enabled: SLAMEM_ERR_ARG.
 *   slamem_stream_set_quals  a -pile stream whose accumulator has quality sums: before the first submit, behind
 *                          slamem_stream_set_pileup.  Every batch then comes through slamem_stream_submit_quals (the other submits
 *                          are refused), which takes the quality bytes beside the letters, indexed as they are (whatever
 *                          offsets[0] is), and the low-quality mask of slamem_stream_submit_masked or NULL (declared with the stream, below). */
int slamem_pileup_enable_quals(slamem_pileup *pile);
int slamem_pileup_quality(slamem_pileup *pile, slamem_pileup **out);
int slamem_pileup_add_quals_device(slamem_pileup *pile, const void *queries_dev, const uint64_t *offsets_dev, uint32_t num_queries,
                                   const slamem_aln *segs_dev, const uint64_t *read_offsets_dev, const uint32_t *ops_dev,
                                   const uint64_t *op_offsets_dev, const slamem_map *reads_dev, uint32_t min_mapq,
                                   const uint64_t *lowq_dev, const uint8_t *quals_dev, uint32_t phred_offset, int dedup,
                                   slamem_map *reads_keep_dev, uint8_t *dup_out_dev, void *stream);
int slamem_pileup_genotypes_weighted_device(slamem_pileup *pile, uint64_t first, uint64_t count, const slamem_gt_params *params,
                                            uint64_t capacity, uint64_t *pos_dev, uint32_t *counts_dev, slamem_genotype *gts_dev,
                                            uint32_t *qsums_dev, uint64_t *total_out, void *stream);
int slamem_pileup_genotypes_weighted_host(slamem_pileup *pile, uint64_t first, uint64_t count, const slamem_gt_params *params,
                                          uint64_t capacity, uint64_t *pos, uint32_t *counts, slamem_genotype *gts, uint32_t *qsums,
                                          uint64_t *total_out);

/* ---- the consensus by genotype likelihood (no option of the front end yet) -------------------------------------------------
 * slamem_pileup_consensus_* with every decision made by the likelihood of -gt.  `row` holds the ploidy, the three costs and the
 * prior of the rows -- what slamem_pileup_genotypes_* would take, -wq's costs when weighted -- and `event` those of the events --
 * what slamem_pileup_genotype_events_* would take; min_depth and min_qual inside the two are not looked at.  A genotype is
 * confident when its GQ, in 64 bits before saturation, is at least 1000 * min_gq.  An event is applied iff its anchor row a (as
 * above) holds one of A,C,G,T, d(a) >= min_depth, and the best genotype of the event against everything else at a is homozygous
 * for it (1/1, or 1 at ploidy 1) and confident; a heterozygous event is not applied.  Row p emits, in this order:
 *   1. and 2. as slamem_pileup_consensus_* over the events applied by this rule;
 *   3. else N if not ACGT(p);
 *   4. else L(p) in lower case if d(p) < min_depth, or A+C+G+T == 0, or the genotype of the row (with its quality sums when
 *      weighted != 0) is not confident;
 *   5. else the best genotype (a, b) in upper case: the letter when a == b, else the IUPAC code of the two (AC M, AG R, AT W,
 *      CG S, CT Y, GT K), also when one of them is L(p).  Ties are those of slamem_pileup_genotypes_*.
 * stats_out has 8 entries: the five of slamem_pileup_consensus_* -- [0] every row of rule 4, [1] rows of rule 5 whose byte is not
 * L(p), an IUPAC code included -- then [5] rows that emit an IUPAC code, [6] rows of rule 4 with d(p) >= min_depth and
 * A+C+G+T > 0 (uncalled for GQ alone), [7] events with first <= pos < first + count whose best genotype is heterozygous and
 * confident, whatever their anchor.  Every range's bytes are a slice of the whole text's and the statistics add up over disjoint
 * ranges.  Capacity, bounds and stream contracts, scratch and what is left unmodified: as slamem_pileup_consensus_*.
 * SLAMEM_ERR_ARG besides: a ploidy, cost or prior outside the ranges of slamem_gt_params, min_depth of 0 or of 2^31 and more,
 * min_gq above 999, weighted above 1, weighted on an accumulator without quality sums. */
typedef struct {
    slamem_gt_params row;   /* ploidy, match_cost, het_cost, err_cost, het_prior of the rows */
    slamem_gt_params event; /* ... of the events */
    uint32_t min_depth;     /* A+C+G+T+D at least this, 1 to 2^31 - 1 */
    uint32_t min_gq;        /* in Phred, 0 to 999 */
    uint32_t weighted;      /* 1: the rows' quality sums count (an accumulator with slamem_pileup_enable_quals) */
} slamem_cons_gt_params;
int slamem_pileup_consensus_gt_device(slamem_pileup *pile, uint64_t first, uint64_t count, const slamem_cons_gt_params *params,
                                      uint64_t capacity, uint8_t *out_dev, const uint64_t *bounds_dev, uint64_t m, uint64_t *offs_dev,
                                      uint64_t *stats_out /* 8 */, uint64_t *total_out, void *stream);
int slamem_pileup_consensus_gt_host(slamem_pileup *pile, uint64_t first, uint64_t count, const slamem_cons_gt_params *params,
                                    uint64_t capacity, uint8_t *out, const uint64_t *bounds, uint64_t m, uint64_t *offs,
                                    uint64_t *stats_out /* 8 */, uint64_t *total_out);

/* ---- (b''''''''''') junctions: long deletions and insertions between segments (option -sv) ---------------------
 * A gap between two chain anchors that -aln does not close ends a segment; the table and the events above hold nothing of what
 * lies between two segments of one read.  With junctions enabled every add of reads also looks at each adjacent pair (a, b) of a
 * contributing read's segments, in ascending order of the scanned strand: dr text rows B and dq read letters A lie between a's end
 * and b's start, m = min(dr, dq), L = |dr - dq|.  Counted and not stored, looked at in this order -- skipped[0]: L == 0 (a
 * divergent stretch, no indel); skipped[3]: m > 64; skipped[2]: a row of B, or a compared letter of A, that is none of A,C,G,T;
 * skipped[3] again: the best split has more than max_mis mismatches; skipped[1]: no room in the table.  The best split shares the
 * m letters out between a's diagonal (the first t) and b's (the rest) with the fewest mismatches, the smallest such t; the
 * junction is then a deletion of L rows from a's end + t (dr > dq) or an insertion of L letters in front of that row (dq > dr),
 * left-normalised by the two rules of the events, without their length limits.  The table maps (pos, kind, len) to fwd and rev as
 * the events' does; the inserted letters are NOT part of the key: two different insertions of one length at one place are one
 * key.  The six columns of the pileup are unchanged: the deleted rows get no D.
 *
 *   slamem_pileup_enable_junctions  allocates the table of `slots` slots (a power of two of at least 64; 0: the smallest power of
 *                          two that is at least max(65536, n / 64)) as slamem_pileup_enable_events does; max_mis: 0 to 64.
 *                          Enabled already, a bad number: SLAMEM_ERR_ARG; too little free HBM: SLAMEM_ERR_NOMEM.
 *                          slamem_pileup_reset also clears this table and its counters.
 *   slamem_pileup_junctions_device  the keys with first <= pos < first + count, fwd + rev >= min_count (>= 1) and len >= min_len,
 *                          ascending in (pos, kind, len), and the four counters; the capacity protocol, the one host round trip
 *                          and the rules about concurrent calls of slamem_pileup_events_device.
 *   slamem_pileup_junctions_host  the same into host memory; waits for the device first.
 *   slamem_pileup_add_junctions_device  every given junction with its fwd and rev: a deletion is validated (inside the text, its
 *                          rows A,C,G,T) and normalised, an insertion (pos < n) is taken where it is given, its letters being no
 *                          part of the record; anything else adds to skipped[2].  The merge of another accumulator's read-out.
 *   slamem_pileup_add_junctions_host  the same from host memory; returns when the junctions are added. */
typedef struct {
    uint64_t pos;
    uint32_t len, fwd, rev;
    uint8_t kind;   /* 0 a deletion of len rows from pos, 1 an insertion of len letters in front of pos */
    uint8_t pad[3]; /* 0 */
} slamem_junction;
int slamem_pileup_enable_junctions(slamem_pileup *pile, uint64_t slots, uint32_t max_mis);
int slamem_pileup_junctions_device(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t min_count, uint32_t min_len,
                                   uint64_t capacity, slamem_junction *junctions_dev, uint64_t *skipped_out /* 4 */,
                                   uint64_t *total_out, void *stream);
int slamem_pileup_junctions_host(slamem_pileup *pile, uint64_t first, uint64_t count, uint32_t min_count, uint32_t min_len,
                                 uint64_t capacity, slamem_junction *junctions, uint64_t *skipped_out /* 4 */, uint64_t *total_out);
int slamem_pileup_add_junctions_device(slamem_pileup *pile, const slamem_junction *junctions_dev, uint64_t m, void *stream);
int slamem_pileup_add_junctions_host(slamem_pileup *pile, const slamem_junction *junctions, uint64_t m);

/* ---- (c) mapping QC tables (-stats) -----------------------------------------------------------------------------
 * A slamem_stats is an accumulator of SLAMEM_STATS_WORDS unsigned 64-bit counters on the index's device, the sum over every batch
 * added since creation or the last reset, whatever the split into batches, their order and their streams: every number is a
 * count.  A read is MAPPED when its record has strand != 0 and COUNTED when it is mapped and mapq >= min_mapq.  The CYCLE of letter
 * x of the scanned strand is x on strand 1 and len - 1 - x on strand 2: the letter's index in the read as given.  A value above a
 * section's last bin goes into that bin.  The sections, as (first word, words):
 *   TOTALS   (0, 24)      16 used: reads; mapped; forward; reverse; counted; counted reads with more than one segment; segments of
 *                         counted reads; letters of all reads; letters of counted reads; letters under =; letters under X; I
 *                         operations; inserted letters; D operations; deleted reference letters; the sum of query_len over the
 *                         segments of counted reads
 *   MAPQ     (24, 64)     mapped reads per mapping quality
 *   LEN      (88, 512)    all reads per length
 *   NM       (600, 128)   counted reads per sum of `edits` over their segments
 *   CYC_ALN  (728, 512)   letters under = or X per cycle          CYC_MM  (1240, 512)  letters under X per cycle
 *   CYC_INS  (1752, 512)  inserted letters per cycle              CYC_DEL (2264, 512)  D operations, at the cycle of the letter of
 *                                                                                      the scanned strand that follows the deletion
 *   SUB      (2776, 16)   per letter under X: 4 * text letter + letter of the scanned strand (A C G T = 0..3); skipped when either
 *                         is none of the four
 *   Q_ALN    (2792, 96)   letters under = or X per quality min(93, max(0, byte - phred_offset)); only with quality bytes
 *   Q_MM     (2888, 96)   letters under X per quality; only with quality bytes
 *   INS_LEN  (2984, 64)   I operations per length                 DEL_LEN (3048, 64)   D operations per length
 * The sections from CYC_ALN on, NM and the TOTALS from `counted` on (but `letters of all reads`) are over the counted reads.  A
 * low-quality mask and the duplicate filter play no part: the table describes the mapping.
 *   slamem_stats_create      the table, all zero; the index must outlive it.  slamem_stats_reset zeroes it (waits for the device).
 *   slamem_stats_add_device  adds the batch that slamem_find_maps_device left behind these pointers: one kernel on `stream`,
 *                            asynchronous, nothing is read back or checked on the host.  quals_dev: a byte per letter, indexed as
 *                            queries_dev is, or NULL (Q_ALN and Q_MM stay as they are).  SLAMEM_ERR_ARG: min_mapq above 60,
 *                            phred_offset above 126, an index without text planes (the COMPACT layout).  Adds from several streams
 *                            and threads into one table are safe: every update is an atomic add.
 *   slamem_stats_table_device / _host  the SLAMEM_STATS_WORDS words; _device is a copy on `stream`, _host waits for the device.
 *   slamem_stats_add_table_host  adds a table to the accumulator (the tables of several GPUs are added up that way).
 *   slamem_stream_set_stats  a stream of match type 7 or 8 adds every batch to `st` (of the stream's device) behind its map pass,
 *                            counting the reads with mapq >= min_mapq; on a stream of type 8 beside the pile add, which is
 *                            untouched.  Before the first submit; SLAMEM_ERR_ARG after it, on another match type, with another
 *                            device's table, with min_mapq above 60 or on an index without text planes.  with_quals != 0: batches
 *                            that come through slamem_stream_submit_quals feed Q_ALN and Q_MM with their bytes (Phred + 33, or the
 *                            offset given to slamem_stream_set_quals); on a type-8 stream this coexists with
 *                            slamem_stream_set_quals, on a type-7 stream it is the only use of the bytes.  A batch that comes
 *                            through another submit has no bytes and leaves the two sections as they are.  A stream that never
 *                            calls it behaves as before and allocates nothing for this (declared with the stream, below). */
#define SLAMEM_STATS_WORDS 3112
typedef struct slamem_stats slamem_stats;
int slamem_stats_create(const slamem_index *idx, slamem_stats **out);
int slamem_stats_free(slamem_stats *st);
int slamem_stats_reset(slamem_stats *st);
int slamem_stats_add_device(slamem_stats *st, const void *queries_dev, const uint64_t *offsets_dev, uint32_t num_queries,
                            const slamem_aln *segs_dev, const uint64_t *read_offsets_dev, const uint32_t *ops_dev,
                            const uint64_t *op_offsets_dev, const slamem_map *reads_dev, const uint8_t *quals_dev /* NULL: none */,
                            uint32_t phred_offset, uint32_t min_mapq, void *stream);
int slamem_stats_table_device(slamem_stats *st, uint64_t *out_dev, void *stream);
int slamem_stats_table_host(slamem_stats *st, uint64_t *out /* SLAMEM_STATS_WORDS */);
int slamem_stats_add_table_host(slamem_stats *st, const uint64_t *table);

/* Host-buffer convenience used by the C front end: uploads the batch, runs
 * slamem_find_mems_device (growing the output buffer if needed) and returns
 * malloc()ed arrays the caller frees with slamem_host_free(). */
int slamem_find_mems_host(const slamem_index *idx, const char *queries, const uint64_t *offsets,
                          uint32_t num_queries, uint32_t min_len, int both_strands,
                          slamem_mem **mems_out, uint64_t **block_offsets_out, uint64_t *total_out);
int slamem_find_mams_host(const slamem_index *idx, const char *queries, const uint64_t *offsets,
                          uint32_t num_queries, uint32_t min_len, int both_strands,
                          slamem_mem **mems_out, uint64_t **block_offsets_out, uint64_t *total_out);
int slamem_find_mums_host(const slamem_index *idx, const char *queries, const uint64_t *offsets,
                          uint32_t num_queries, uint32_t min_len, int both_strands,
                          slamem_mem **mems_out, uint64_t **block_offsets_out, uint64_t *total_out);
int slamem_find_smems_host(const slamem_index *idx, const char *queries, const uint64_t *offsets,
                           uint32_t num_queries, uint32_t min_len, int both_strands, uint32_t max_occ,
                           slamem_mem **mems_out, uint64_t **block_offsets_out, uint64_t *total_out);
/* (block_scores_out may be NULL; otherwise a third malloc()ed array, a uint32 per strand block) */
int slamem_find_chains_host(const slamem_index *idx, const char *queries, const uint64_t *offsets,
                            uint32_t num_queries, uint32_t min_len, int both_strands, uint32_t max_gap,
                            slamem_mem **mems_out, uint64_t **block_offsets_out, uint32_t **block_scores_out,
                            uint64_t *total_out);
/* (mismatches_out may be NULL; otherwise a third malloc()ed array, a uint32 per returned row) */
int slamem_find_exts_host(const slamem_index *idx, const char *queries, const uint64_t *offsets,
                          uint32_t num_queries, uint32_t min_len, int both_strands, uint32_t mismatch_penalty, uint32_t xdrop,
                          slamem_mem **mems_out, uint64_t **block_offsets_out, uint32_t **mismatches_out,
                          uint64_t *total_out);
/* (four malloc()ed arrays: segments, num_blocks + 1 block offsets, operations, segments + 1 operation offsets;
 * totals_out[0..2] as for slamem_find_alns_device) */
int slamem_find_alns_host(const slamem_index *idx, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                          uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                          uint32_t max_edits, slamem_aln **segs_out, uint64_t **block_offsets_out, uint32_t **ops_out,
                          uint64_t **op_offsets_out, uint64_t *totals_out);
/* (five malloc()ed arrays: segments, num_queries + 1 read offsets, operations, segments + 1 operation offsets, num_queries
 * read records; totals_out[0..2] as for slamem_find_alns_device) */
int slamem_find_maps_host(const slamem_index *idx, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                          uint32_t min_len, int both_strands, uint32_t max_gap, uint32_t mismatch_penalty, uint32_t xdrop,
                          uint32_t max_edits, slamem_aln **segs_out, uint64_t **read_offsets_out, uint32_t **ops_out,
                          uint64_t **op_offsets_out, slamem_map **reads_out, uint64_t *totals_out);
void slamem_host_free(void *p);

/* ---- (b') MEM retrieval, host to host, pipelined -------------------------------
 * The query loop of GetMatches (slamem.c:90-207) for a front end whose reads live in HOST memory -- the boundary SURVEY.md
 * 8(d) defines the path's metric on.  A stream is a three-stage pipeline (upload, search, download: one host thread
 * and one HIP stream each) over `slots` (2..8) sets of device + pinned result buffers: while the search kernels of batch b
 * run, the copy engines upload batch b+1 and download the MEMs of batch b-1, so the sustained rate is the kernels' rate,
 * not kernels + PCIe.  Four or five slots keep all three stages busy beside the result the caller is working on.
 *
 *   slamem_stream_create   max_batch_chars / max_batch_queries: what to reserve per slot (a larger batch makes its slot
 *                          grow); match_type 0 = MEM, 1 = MAM (-mam), 2 = MUM (-mum:
 *                          only the kept rows come back), 3 = SMEM (-smem: likewise), 4 = chain (-chain: likewise; rows
 *                          and offsets, no scores), 5 = extension (-ext: the extended rows; their mismatches through
 *                          slamem_stream_mismatches), 6 = alignment (-aln: slamem_stream_next gives the block offsets and, as
 *                          its total, the number of segments -- its rows pointer is not to be read; the segments, operations
 *                          and operation offsets come through slamem_stream_alns), 7 = mapping (-paf: as 6 with the offsets
 *                          per READ, num_queries + 1 of them, and a record per read through slamem_stream_maps; it takes the
 *                          setters of 6), 8 = pileup (-pile: every batch goes the way of 7 and is then added to the accumulator
 *                          given with slamem_stream_set_pileup, on the device; its segments and operations stay there and are
 *                          NOT downloaded.  slamem_stream_next gives the number of segments piled as its total -- its rows and
 *                          offsets pointers are not to be read --, slamem_stream_maps the read records; slamem_stream_alns is
 *                          SLAMEM_ERR_ARG.  It takes the setters of 7.  When slamem_stream_next hands a batch back its reads
 *                          are in the table.)
 *   slamem_stream_set_pileup  -pile: the accumulator every batch is added to and the least mapping quality that counts (0 to
 *                          60); before the first submit.  SLAMEM_ERR_ARG after it, on a stream of another match type, with an
 *                          accumulator of another device, or with a quality above 60; a submit on a stream of match type 8
 *                          that has no accumulator is SLAMEM_ERR_ARG too.  Several streams of one device may share one
 *                          accumulator: every update is an atomic add.  The add is enqueued once the batch's totals have shown
 *                          that its result stands (a batch that is run again with more room is piled once).
 *   slamem_stream_set_max_occ  -smem: the occurrence cap of every batch (0: none, the default); before the first submit
 *                          (SLAMEM_ERR_ARG after it, or with a cap on a stream of another match type)
 *   slamem_stream_set_max_gap  -chain: the maximum gap of every batch (0: the default 5000); before the first submit
 *                          (SLAMEM_ERR_ARG after it, with a gap on a stream of another match type, or from 2^31)
 *   slamem_stream_set_ext_params  -ext: mismatch penalty (0: the default 4) and X-drop (SLAMEM_EXT_XDROP_DEFAULT: the default
 *                          20) of every batch; before the first submit (SLAMEM_ERR_ARG after it, or with values other than the
 *                          defaults' placeholders on a stream of another match type)
 *   slamem_stream_mismatches  -ext: the mismatches (a uint32 per row) of the batch slamem_stream_next returned last, in the
 *                          stream's pinned memory; valid as long as that batch's rows.  The same for submit and submit_packed.
 *   slamem_stream_set_max_edits  -aln: the most edits in one gap of every batch (SLAMEM_ALN_EDITS_DEFAULT: the default 31; at
 *                          most 127); before the first submit.  A stream of match type 6 also takes slamem_stream_set_max_gap
 *                          and slamem_stream_set_ext_params, for its chain and its outer ends.
 *   slamem_stream_alns     -aln: segments, operations, operation offsets (segments + 1) and the number of operations of the
 *                          batch slamem_stream_next returned last, in the stream's pinned memory; valid as long as that batch.
 *   slamem_stream_submit   record i of the batch is queries[offsets[i] .. offsets[i+1]) -- offsets[0] need not be 0, so
 *                          a front end passes its whole character buffer and a window of its offsets array.  Returns at
 *                          once; the characters and offsets must stay unchanged until the batch has been collected.
 *                          Uploads run at full PCIe rate when `queries` AND `offsets` are pinned memory
 *                          (slamem_pinned_alloc): 8 bytes of offsets per record go up with every batch.
 *                          Never blocks: SLAMEM_ERR_ARG when every slot is in use.
 *   slamem_stream_next     waits for the OLDEST submitted batch (results come back in submission order) and lends its
 *                          result: mems grouped by strand block in the reference's emission order and block offsets,
 *                          laid out as slamem_find_mems_device does, in pinned host memory owned by the stream, valid
 *                          until the next slamem_stream_next / slamem_stream_destroy call.  A failed batch returns its
 *                          error code here.  So one thread keeps slots - 1 batches in flight beside the one it works on:
 *                              submit(0..slots-2);  for b: next(b); submit(b + slots - 1); use result b
 *   slamem_stream_destroy  waits for the batches in flight, then frees everything.
 * No CPU fallback: every batch is searched on the GPU. */
typedef struct slamem_stream slamem_stream;
int slamem_stream_create(const slamem_index *idx, int slots, uint64_t max_batch_chars, uint32_t max_batch_queries,
                         int both_strands, int match_type, slamem_stream **out);
int slamem_stream_set_max_occ(slamem_stream *s, uint32_t max_occ);
int slamem_stream_set_max_gap(slamem_stream *s, uint32_t max_gap);
int slamem_stream_set_ext_params(slamem_stream *s, uint32_t mismatch_penalty, uint32_t xdrop);
int slamem_stream_mismatches(slamem_stream *s, const uint32_t **out);
int slamem_stream_set_max_edits(slamem_stream *s, uint32_t max_edits);
/* -gext: the band of the gapped outer ends, after slamem_stream_set_max_edits and before the first submit */
int slamem_stream_set_end_band(slamem_stream *s, uint32_t end_band);
int slamem_stream_alns(slamem_stream *s, const slamem_aln **segs_out, const uint32_t **ops_out, const uint64_t **op_offsets_out,
                       uint64_t *num_ops_out);
/* -paf, -pile: the read records (num_queries of them) of the batch slamem_stream_next returned last, in the stream's pinned memory;
 * valid as long as that batch.  Its segments and operations come through slamem_stream_alns. */
int slamem_stream_maps(slamem_stream *s, const slamem_map **reads_out);
int slamem_stream_set_pileup(slamem_stream *s, slamem_pileup *pile, uint32_t min_mapq);
/* -dedup (described with slamem_pileup_enable_dedup above) */
int slamem_stream_set_dedup(slamem_stream *s, int on);
int slamem_stream_dups(slamem_stream *s, const uint8_t **flags_out);
/* -wq (described with slamem_pileup_enable_quals above) */
int slamem_stream_set_quals(slamem_stream *s, uint32_t phred_offset);
int slamem_stream_submit_quals(slamem_stream *s, const char *queries, const uint8_t *quals, const uint64_t *lowq,
                               const uint64_t *offsets, uint32_t num_queries, uint32_t min_len);
/* -stats (described with slamem_stats_create above) */
int slamem_stream_set_stats(slamem_stream *s, slamem_stats *st, uint32_t min_mapq, int with_quals);
/* -sam: on != 0 makes every slot of a stream of match type 7 run slamem_maps_md_device behind its batch and
 * download the four arrays; before the first submit (SLAMEM_ERR_ARG after it, or on a stream of another match type).  A stream
 * that never calls it behaves as before and allocates nothing for this.  slamem_stream_md gives the arrays of the batch
 * slamem_stream_next returned last, in the stream's pinned memory, valid as long as that batch: *num_md_out entries, segments + 1
 * offsets, a uint32 per segment, a uint32 per read.  SLAMEM_ERR_ARG on a stream whose MD pass is not switched on. */
int slamem_stream_set_md(slamem_stream *s, int on);
int slamem_stream_md(slamem_stream *s, const uint32_t **md_out, const uint64_t **md_offsets_out, const uint32_t **seg_eq_out,
                     const uint32_t **primary_out, uint64_t *num_md_out);
int slamem_stream_submit(slamem_stream *s, const char *queries, const uint64_t *offsets, uint32_t num_queries,
                         uint32_t min_len);
/* -pile with a low-quality mask: slamem_stream_submit for a stream of match type 8, with `lowq` indexed as
 * `queries` is -- bit offsets[i] + k is letter k of record i, whatever offsets[0] is.  The stream uploads the words that hold a
 * bit of the batch and adds the batch with slamem_pileup_add_masked_device's kernels; lowq must stay unchanged as queries must.
 * lowq NULL: slamem_stream_submit.  A stream of another match type: SLAMEM_ERR_ARG.  slamem_stream_submit and
 * slamem_stream_submit_packed on the same stream remain the unmasked ones. */
int slamem_stream_submit_masked(slamem_stream *s, const char *queries, const uint64_t *lowq, const uint64_t *offsets,
                                uint32_t num_queries, uint32_t min_len);
/* The same for reads the caller holds PACKED (ABI 4; no reference counterpart: the reference reads letters, sequence.c:89-270).
 * Since the search takes ~9 ms for 10 M reads the link bounds this path (1.5 GB of letters: 26 ms); packed reads are a third.
 *   planes   16-byte units {p0, p1} (two 64-bit words): bit i of p0 / p1 = low / high bit of letter 64u+i of the record
 *            (A,C,G,T = 0..3; a letter that is none of them: 0 and its bit in `other`).  A record starts a new unit: record i
 *            of `len` letters takes (len + 63) / 64 units, the units of the batch's records follow each other.
 *   other    per unit: bit i = letter 64u+i is not one of A,C,G,T (it is searched as N, sequence.c:61-81); NULL: no such letter
 *   offsets  as for slamem_stream_submit (in letters; only differences are used)
 *   num_units  the units of the batch (slamem_pack_reads counts them), or 0: counted from the offsets (1 ms per million records)
 * slamem_pack_reads makes the two arrays from letters (host, `threads` threads; units_out: their number).  16-byte aligned
 * `planes`; pinned memory for full link rate. */
int slamem_stream_submit_packed(slamem_stream *s, const void *planes, const uint64_t *other, const uint64_t *offsets,
                                uint32_t num_queries, uint64_t num_units, uint32_t min_len);
int slamem_pack_reads(const char *queries, const uint64_t *offsets, uint32_t num_queries, void *planes_out, uint64_t *other_out,
                      uint64_t *units_out, int threads);
int slamem_stream_next(slamem_stream *s, const slamem_mem **mems_out, const uint64_t **block_offsets_out,
                       uint64_t *total_out, uint32_t *num_queries_out, slamem_timings *timings_out);
int slamem_stream_destroy(slamem_stream *s);
/* Page-locked host memory for a front end's read buffers (hipHostMalloc / hipHostFree). */
int slamem_pinned_alloc(void **out, uint64_t bytes);
int slamem_pinned_free(void *p);
/* hipMemcpy device -> host (for a front end that fills its pinned buffers from device memory). */
int slamem_copy_to_host(void *dst_host, const void *src_dev, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SLAMEM_HIP_H */
