/* slamem_host.h -- host side of the slaMEM-compatible front end (plain C, no GPU code).
 *
 * Written from scratch against the reference's observable behaviour:
 *   - FASTA loading / normalisation / merging        sequence.c:61-81, 89-270, 272-301, 309-320
 *   - command-line conventions                        slamem.c:528-663, tools.c:31-79
 *   - the *-mems.txt text format                      slamem.c:98, 102, 144-148
 * libslamem_host.so carries these for the CPU tests; slaMEM-hip links them with libslamem_hip.so.
 */
#ifndef SLAMEM_HOST_H
#define SLAMEM_HOST_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    char *name;    /* full header line after '>' (sequence.c:213-217) */
    uint32_t size; /* normalised characters of this record            */
} slh_record;

typedef struct {
    slh_record *recs;
    int num;                /* accepted records                                                      */
    char *chars;            /* merge: rec0 'N' rec1 'N' ... ; otherwise the records back to back     */
    uint64_t total;         /* bytes in chars (merge: what the reference stores as allSequences[0]->size) */
    uint64_t *offsets;      /* !merge: num+1 start offsets into chars                                */
    uint32_t *merged_start; /* merge: start of record k in chars (sequence.c:260-262)                */
    long file_bytes;
    void *name_arena;       /* owns the name strings */
} slh_seqset;

/* LoadSequencesFromFile (sequence.c:89-270).  merge=1 for the reference file (records joined by 'N',
 * name filter applies), merge=0 for query files.  first_number: running record number for the
 * "# NN [name]" log lines; log may be NULL.  log_limit: at most this many per-record lines are printed
 * (the reference prints all; 0 = unlimited).  Returns the number of accepted records, 0 on any failure
 * (message printed to log like the reference does). */
int slh_load_file(const char *path, int merge, int acgt_only, uint32_t min_len, const char *name_filter,
                  int first_number, long log_limit, slh_seqset *out, FILE *log);
void slh_free_seqset(slh_seqset *s);
/* The same for a file that may be FASTQ (its first byte is '@'): four lines a record -- '@' and the name, kept
 * as FASTA keeps what follows '>'; the letters; a line that starts with '+'; as many quality bytes as the second line has letter
 * bytes; "\r\n" is accepted.  The letters go through the FASTA rules, and a letter they drop drops its quality byte with it.
 * *quals_out (release with free()) is parallel to out->chars: the quality byte of every kept letter, as the file has it; NULL for
 * a FASTA file, and quals_out may be NULL (the qualities are dropped).  slh_seqset is as it was: callers mirror its layout.
 * Returns -1, with "> ERROR: Invalid FASTQ file" on the log, for a file that breaks the four-line rule (a first byte that is no
 * '@', a third line without '+', unequal lengths, a last record cut short), and -1 with a message of its own for merge=1: the
 * reference file stays FASTA.  A FASTA file: exactly slh_load_file. */
int slh_load_file_q(const char *path, int merge, int acgt_only, uint32_t min_len, const char *name_filter,
                    int first_number, long log_limit, slh_seqset *out, char **quals_out, FILE *log);
/* A query file handed out in consecutive pieces of about piece_bytes of the file each (the same records as
 * slh_load_file(path, 0, ...) would give in one set): a front end searches the first reads while the rest is parsed. */
typedef struct slh_pieces slh_pieces;
slh_pieces *slh_pieces_open(const char *path, int acgt_only, uint32_t min_len, int first_number, long log_limit,
                            long piece_bytes, FILE *log);
int slh_pieces_next(slh_pieces *p, slh_seqset *out); /* records in the piece; 0 at the end */
/* the same for a file that may be FASTQ: *quals_out as for slh_load_file_q (NULL for FASTA), -1 for an invalid FASTQ file.  A
 * FASTQ file is cut into pieces, and a piece into the parser threads' shares, by counting lines from a known record start: a '@'
 * behind a newline may begin a quality line. */
int slh_pieces_next_q(slh_pieces *p, slh_seqset *out, char **quals_out);
void slh_pieces_close(slh_pieces *p);
/* on: the page-cache mapping of every parsed piece is dropped at once (for inputs whose footprint matters more than the
 * address-space work this causes beside the other threads; off by default) */
void slh_pieces_release_parsed(slh_pieces *p, int on);
/* malloc for buffers of tens of MB and more: 2 MB aligned, marked for transparent huge pages; release with free() */
void *slh_big_malloc(size_t bytes);
/* host threads used for loading / formatting: SLAMEM_THREADS or the online CPUs, at most 32 */
int slh_thread_count(void);

/* GetSeqIdFromMergedSeqsPos (sequence.c:309-320). */
int slh_seq_id_from_merged_pos(const uint32_t *starts, int num, uint32_t *pos);

/* The walk of the read-outs over a merged text that is read in ranges of rows: the next piece of a record inside the range that
 * ends in front of row range_end.  *r is the record to look at first (0 before the first range) and *x the row the walk has
 * reached (the range's first row before its first piece); both move on, *r only past a record whose last row was handed out,
 * so the next range goes on where this one stopped.  The separators between the records belong to no piece.  Returns 1 and the
 * piece -- rows [a, b) of record rec, which starts at row `start`; ends_record: b is the record's end -- or 0 when the range
 * holds no further piece. */
typedef struct {
    int rec, ends_record;
    uint64_t start, a, b;
} slh_piece;
int slh_next_piece(const slh_record *recs, const uint32_t *merged_start, int num, int *r, uint64_t *x, uint64_t range_end,
                   slh_piece *out);

/* Options as the reference parses them (slamem.c:571-663; tools.c:31-62). */
typedef struct {
    int usage;          /* argc < 3                                          */
    int hidden_sort;    /* -s given: slh_sort_mems_file                      */
    int hidden_clean;   /* -c given: slh_clean_fasta                         */
    int image_arg;      /* index of the -v value, or -1: slh_mem_map_image   */
    int no_ns;          /* -n                                                */
    int min_seq_len;    /* -m, 0 if absent                                   */
    char *ref_name;     /* -r string (malloc'ed) or NULL                     */
    int ref_name_given; /* -r present                                        */
    int ref_name_empty; /* -r present without a string                       */
    int match_type;     /* 0 MEM, 1 MAM (-ma...), 2 MUM (-mu...), 3 SMEM (-sm...), 4 chain (-ch...), 5 extension (-ex...), 6 alignment (-al...), 7 mapping (-pa..., and -sa...: the same written as SAM), 8 pileup (-pi..., and -si...: its variant sites, -vc...: its calls as VCF), -1 two of them */
    int both_strands;   /* -b                                                */
    int min_mem_len;    /* -l, default 20                                    */
    int out_arg;        /* index of the -o value, or -1                      */
    int num_files;
    int *file_args;     /* indices into argv of the FASTA files, in order    */
} slh_options;

int slh_parse_options(int argc, char **argv, slh_options *o);
void slh_free_options(slh_options *o);
/* ParseArgument (tools.c:31-62) */
int slh_parse_argument(int argc, char **argv, const char *optionchars, int parse);
/* The options behind the reference's are rows of one table in slamem_host.c: the first two letters decide, either case (-maxed
 * and -dedup: three, because "-ma" is -mam and "-de" -depth), and the value of a row that takes one is never a file name.  Row k
 * of the table: its name in *name_out and whether it takes a value, or -1 behind the last row. */
int slh_option_info(int k, const char **name_out);
/* The values, one entry point per group of options (not fields of slh_options, whose layout callers mirror).  An entry point with
 * one option returns 0 when it is absent (the default in the output), 1 when it is there, -1 when its value is missing, no whole
 * number or out of range; only the first occurrence is looked at.  One with several looks at every occurrence, the last one
 * counts, and returns 0, 1 when any is there, or -k when the value of its k-th option is refused.
 *   -occ N >= 1 (default 0); -mgap N >= 1 (0); -maxed N in [0, 127] (-1); -minq N in [0, 60] (0); -bq N in [0, 93] (0);
 *   -evs N, a power of two in [64, 2^31] (0) */
int slh_parse_max_occ(int argc, char **argv, int *out);
int slh_parse_max_gap(int argc, char **argv, int *out);
int slh_parse_max_edits(int argc, char **argv, int *out);
/* -affine X,O,E: 0 absent, 1 there with the three costs, -1 refused; the max_edits word the library takes
 * (SLAMEM_ALN_AFFINE; max_edits < 0: the default), and that word's fields E, x, o, e with the rule it breaks (0: none) */
int slh_parse_affine(int argc, char **argv, int *x_out, int *o_out, int *e_out);
uint32_t slh_aln_word(int max_edits, int affine, int x, int o, int e);
/* -gext Z: 0 absent (*out = 0), 1 there with the band 1..31, -1 refused */
int slh_parse_gext(int argc, char **argv, int *out);
int slh_aln_word_decode(uint32_t word, uint32_t *fields_out, int *affine_out);
int slh_parse_min_mapq(int argc, char **argv, int *out);
int slh_parse_min_bq(int argc, char **argv, int *out);
int slh_parse_event_slots(int argc, char **argv, uint64_t *out);
/* -pen N >= 1 (0) and -xdrop N >= 0 (-1): -1 for either */
int slh_parse_ext_params(int argc, char **argv, int *penalty_out, int *xdrop_out);
/* -mdep N >= 1 (4) and -mpct P in [0, 100] (20): -1 and -2 */
int slh_parse_sites_params(int argc, char **argv, int *min_depth_out, int *min_pct_out);
/* -ploidy 1|2 (2), -err Q in [1, 93] (20), -hetq N in [0, 999] (30), -qual N in [0, 999] (20): -1 to -4 */
int slh_parse_gt_params(int argc, char **argv, int *ploidy_out, int *err_out, int *hetq_out, int *qual_out);
/* -sb and -fs N in [0, 999] (-1: absent): bit 0 of the result says that -sb is there, bit 1 that -fs is; -1 when the value of -fs
 * is refused */
int slh_parse_sb_params(int argc, char **argv, int *fs_out);
/* -wq (no value; needs -gt): whether it is there */
int slh_parse_wq(int argc, char **argv);
/* -stats (no value; a mode of its own that runs as -paf does and takes -minq): whether it is there */
int slh_parse_stats(int argc, char **argv);
/* -depth: is it given? */
int slh_parse_depth(int argc, char **argv);
/* -dedup and -dslots N, a power of two in [64, 2^32] (0): bit 0 of the result says that -dedup is there, bit 1 that -dslots is;
 * -1 when the value of -dslots is refused */
int slh_parse_dedup(int argc, char **argv, uint64_t *slots_out);
/* -lev LIST and -win N >= 1 (0): LIST is 1 to 16 whole numbers in [1, 2^32), strictly ascending, separated by commas (levels_out
 * has room for 16); both begin with a digit.  Bit 0 of the result says that -lev is there, bit 1 that -win is; -1 and -2 */
int slh_parse_depth_params(int argc, char **argv, uint32_t *levels_out, int *num_levels_out, uint64_t *window_out);
/* Everything the command line says, for main(): slh_options and the values of the entry points above, with the switches. */
typedef struct {
    slh_options o;
    int max_occ, max_gap, ext_pen, ext_xdrop, max_edits, min_mapq;
    int min_bq, bq_given; /* (what slh_parse_min_bq returned) */
    int min_depth, min_pct; /* (-depth without -mdep: min_depth = 1) */
    uint64_t ev_slots, dd_slots;
    uint32_t levels[16];
    int num_levels;
    uint64_t window;
    int gt_ploidy, gt_err, gt_hetq, gt_qual;
    int sites, vcf, cons, depth, sam, dedup, gt;
} slh_run;
/* Parses, then refuses: bad values, an option without the mode it belongs to, modes that exclude each other -- the first that
 * applies, its message in *refusal.  Returns 0 (accepted, or o.usage / o.hidden_sort / o.hidden_clean is set and nothing was
 * refused), -1 (refused), or -2 (refused for too few files or an empty -r string: the caller first makes the checks that need
 * more than the arguments).  Release out->o with slh_free_options. */
int slh_parse_run(int argc, char **argv, slh_run *out, const char **refusal);
/* AppendToBasename (tools.c:65-79): everything before the last '.' of the whole path + extra */
char *slh_append_to_basename(const char *filename, const char *extra);

/* One strand block of the output file (slamem.c:98/102 header + :144-148 lines).
 * mems: triples (ref_pos, query_pos, length), 0-based; printed 1-based.  When num_refs > 1 every line is
 * prefixed by " <record name>\t" and ref_pos is made relative to the record.  Appends to buf (realloc'ed). */
typedef struct {
    char *data;
    size_t len, cap;
} slh_buffer;
int slh_format_block(slh_buffer *buf, const char *query_name, int reverse, const uint32_t *mems, uint64_t count,
                     const slh_record *refs, const uint32_t *merged_start, int num_refs, uint64_t *sum_len_out);
/* The same with a fourth column (-ext: the mismatches of each row): extra[i] is printed behind the length of row i, as it
 * is; extra == NULL: slh_format_block. */
int slh_format_block_ext(slh_buffer *buf, const char *query_name, int reverse, const uint32_t *mems, const uint32_t *extra,
                         uint64_t count, const slh_record *refs, const uint32_t *merged_start, int num_refs,
                         uint64_t *sum_len_out);
/* A strand block of the -aln file: the -mem header, then per segment ref_pos query_pos ref_len query_len edits cigar, the
 * positions as -mem prints them.  segs: five uint32 per segment; op_off[i] .. op_off[i + 1]: segment i's operations in ops
 * (length << 4 | BAM code of = X I D).  *sum_len_out: the query letters of the segments. */
int slh_format_block_aln(slh_buffer *buf, const char *query_name, int reverse, const uint32_t *segs, const uint32_t *ops,
                         const uint64_t *op_off, uint64_t count, const slh_record *refs, const uint32_t *merged_start,
                         int num_refs, uint64_t *sum_len_out);
/* A read of the -paf file (plain PAF, no header lines): one line per segment, in the segments' order,
 *   name  read_len  qs  qe  +|-  record  record_len  ts  te  letters under =  all operation lengths  mapq  NM:i:  s1:i:  s2:i:  cg:Z:
 * both names cut at the first blank or tab; qs, qe on the read as given (strand 2, the reverse strand: qs = read_len -
 * query_pos - query_len); ts, te local to the record that holds the segment's first reference letter.  strand 0 (an unmapped
 * read) and count 0 write nothing.  segs, ops, op_off as for slh_format_block_aln.  *sum_len_out: the query letters of the
 * segments. */
int slh_format_read_paf(slh_buffer *buf, const char *query_name, uint32_t query_len, int strand, uint32_t mapq, uint32_t s1,
                        uint32_t s2, const uint32_t *segs, const uint32_t *ops, const uint64_t *op_off, uint64_t count,
                        const slh_record *refs, const uint32_t *merged_start, int num_refs, uint64_t *sum_len_out);
/* A read of the -sam file.  A read with strand 0 or count 0 gets one line, `name 4 * 0 0 * * 0 0 SEQ QUAL`;
 * any other one line per segment, in the segments' order:
 *   name  FLAG  record  ts + 1  mapq  CIGAR  *  0  0  SEQ  QUAL  NM:i:  MD:Z:  s1:i:  s2:i:  [SA:Z:]
 * FLAG = 16 on strand 2 | 2048 on every segment but number `primary`; the CIGAR is <query_pos>S, the operations, <n - query_pos
 * - query_len>S (a clip of 0 is left out), so every line carries the whole read; SEQ is the n letters as given, on strand 2
 * their reverse complement by the engine's rule (A<->T, C<->G, anything else N); QUAL the n quality bytes, reversed on strand 2,
 * `*` when quals is NULL.  md, md_off: the MD entries of slamem_maps_md_device, md_off[i] .. md_off[i + 1] those of segment i.
 * With more than one segment SA:Z: lists `record,pos,+|-,CIGAR,mapq,NM;` of the others.  segs, ops, op_off, names,
 * *sum_len_out as for slh_format_read_paf.  slh_format_sam_header: @HD, an @SQ per record, @PG (no CL:). */
int slh_format_read_sam(slh_buffer *buf, const char *query_name, const char *letters, const char *quals, uint32_t n, int strand,
                        uint32_t mapq, uint32_t s1, uint32_t s2, const uint32_t *segs, const uint32_t *ops, const uint64_t *op_off,
                        const uint32_t *md, const uint64_t *md_off, uint32_t primary, uint64_t count, const slh_record *refs,
                        const uint32_t *merged_start, int num_refs, uint64_t *sum_len_out);
int slh_format_sam_header(slh_buffer *buf, const slh_record *refs, int num_refs);
/* Rows of the -pile file: one line per row with a non-zero counter,
 *   record name (cut at the first blank or tab)  position  reference letter (upper case)  A  C  G  T  D  I
 * counts: six uint32 per row; letters[i]: the reference letter of row i; first_pos: the 1-based position of row 0 in its record. */
int slh_format_pile_rows(slh_buffer *buf, const char *record_name, uint32_t first_pos, const char *letters, const uint32_t *counts,
                         uint64_t rows);
/* Rows of the -sites file: one line per row given,
 *   record name (cut at the first blank or tab)  position  reference letter (upper case)  A  C  G  T  D  I  calls
 * pos[i]: the row's position in the merged text (inside the record, which starts at record_start), text: the merged text,
 * counts: six uint32 per row, alleles[i]: the row's mask; calls: its set bits in the order A C G T D I, joined by commas. */
int slh_format_site_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, const char *text, const uint64_t *pos,
                         const uint32_t *counts, const uint8_t *alleles, uint64_t rows);
/* The head of the -vcf file: ##fileformat=VCFv4.2, a ##contig line per record (the name cut at the first blank or tab), the
 * ##INFO lines of DP, AO, SF and SR and the #CHROM line. */
int slh_format_vcf_header(slh_buffer *buf, const slh_record *refs, int num_refs);
/* An indel event as the engine reads it out (the layout of slamem_event): kind 0 a deletion of len rows from pos, 1 an insertion
 * of len letters in front of pos; letters: two bits a letter (A C G T = 0..3), letter i at bits 2 * (len - 1 - i). */
typedef struct {
    uint64_t pos;
    uint64_t letters;
    uint32_t fwd, rev;
    uint8_t kind, len;
    uint8_t pad[6];
} slh_event;
/* Lines of the -vcf file for one record (record_start in the merged text, record_size letters): the SNVs of the given -sites
 * rows (a line per set bit of A C G T: REF the text's letter, ALT the bit's letter, DP=depth;AO=count) and the given events that
 * are called -- anchor_rows[6 e ..]: the pileup row of event e's anchor (pos - 1, or pos at the record's first letter); called iff
 * its depth d >= min_depth and 100 (fwd + rev) >= min_pct d.  A deletion is written as anchor + deleted rows -> anchor, an
 * insertion as anchor -> anchor + letters; at the record's first letter the following base anchors (VCF 4.2), and a deletion
 * that reaches the record's end gives no line.  Both lists ascend and lie inside the record; the lines are sorted by POS, at one
 * POS the SNVs first. */
int slh_format_vcf_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                        const uint64_t *site_pos, const uint32_t *site_counts, const uint8_t *site_alleles, uint64_t sites,
                        const slh_event *events, const uint32_t *anchor_rows, uint64_t num_events, uint32_t min_depth,
                        uint32_t min_pct);
/* -vcf -sv.  -sv and its values -svmin N (>= 1; *min_len_out -1 when absent: maxed + 1), -svmis N (0 to 64,
 * default 3) and -svslots N (a power of two in [64, 2^31], 0 when absent): the options seen as bits 0..3 in this order, or
 * -2, -3, -4 when the value of -svmin, -svmis, -svslots is refused. */
int slh_parse_sv(int argc, char **argv, int *min_len_out, int *max_mis_out, uint64_t *slots_out);
/* A junction as the engine reads it out (the layout of slamem_junction). */
typedef struct {
    uint64_t pos;
    uint32_t len, fwd, rev;
    uint8_t kind;
    uint8_t pad[3];
} slh_junction;
/* The head of the -vcf -sv file: that of -vcf with the ##ALT lines of DEL and INS and the ##INFO lines of SVTYPE, END and SVLEN
 * in front of the column line. */
int slh_format_vcf_sv_header(slh_buffer *buf, const slh_record *refs, int num_refs);
/* slh_format_vcf_rows with the record's junctions (ascending in pos, kind, len; jrows[6 j ..]: the pileup row of junction j's
 * anchor pos - 1): a junction is called by the events' rule at its anchor and written, with x the anchor's position in the record,
 * as POS x, REF the anchor's letter, ALT <DEL> with SVTYPE=DEL;END=x+len;SVLEN=-len or ALT <INS> with SVTYPE=INS;END=x;SVLEN=len,
 * then DP, AO, SF, SR; at one POS behind the SNVs and the events.  A junction at the record's first row has no anchor and gives
 * no line.  counts_out[0] += the junction lines written, counts_out[1] += the junctions at a first row. */
int slh_format_vcf_sv_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const uint8_t *site_alleles, uint64_t sites,
                           const slh_event *events, const uint32_t *anchor_rows, uint64_t num_events, const slh_junction *junctions,
                           const uint32_t *jrows, uint64_t num_junctions, uint32_t min_depth, uint32_t min_pct, uint64_t *counts_out);
/* -vcf -gt.  A genotype as the engine writes it (the layout of slamem_genotype): scores in milli-Phred, a <= b
 * letter columns (SNV) or allele numbers 0 / 1 (event), pl by genotype number. */
typedef struct {
    uint32_t qual, gq;
    uint8_t a, b, ploidy, ref;
    uint32_t pl[10];
    uint8_t pad[4];
} slh_genotype;
/* The head of the -vcf -gt file: that of -vcf with AO as Number=A, the ##FORMAT lines of GT, DP, AD, GQ and PL, and the columns
 * FORMAT and sample behind INFO. */
int slh_format_vcf_gt_header(slh_buffer *buf, const slh_record *refs, int num_refs);
/* Lines of the -vcf -gt file for one record: a line per given site (the rows slamem_pileup_genotypes_* selected) -- ALT the best
 * genotype's letters other than the reference's, ascending; QUAL (qual + 500) / 1000; DP=depth;AO= the ALT counts; the sample
 * column GT:DP:AD:GQ:PL with the alleles numbered over REF, ALT, joined by / (one number at ploidy 1), GQ at most 99, PL the
 * line's genotypes in VCF order minus their own minimum, rounded as QUAL is -- and a line per given event whose called[e] is
 * not 0: the line of slh_format_vcf_rows with QUAL and the sample column (AD = ro, ao).  Order and the rule at a record's end as
 * there. */
int slh_format_vcf_gt_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const slh_genotype *site_gts, uint64_t sites,
                           const slh_event *events, const uint32_t *anchor_rows, const slh_genotype *event_gts, const uint8_t *called,
                           uint64_t num_events);
/* -vcf -gt -sb.  The head of -vcf -gt with ##INFO FS behind its INFO lines, ##FORMAT SB behind its FORMAT lines
 * and, when fs_filter >= 0 (-fs N), ##FILTER sb in front of the INFO lines. */
int slh_format_vcf_sb_header(slh_buffer *buf, const slh_record *refs, int num_refs, int fs_filter);
/* The lines of slh_format_vcf_gt_rows, each with its strand table (rf, rr, af, ar: reference forward and reverse, alternative
 * forward and reverse) as a sixth sample value SB, ;FS= its slamem_fisher.h value with three decimals behind INFO, and with
 * fs_filter >= 0 FILTER sb when FS > fs_filter, else PASS.  site_fwd, anchor_fwd: the rows of the forward accumulator at the
 * sites and at the events' anchors.  SNV, r the reference column: rf = fwd[r], rr = row[r] - fwd[r], af and ar the same summed
 * over the line's ALT letters.  Event: af = fwd, ar = rev of the event, and with d, df the depths A+C+G+T+D of the two rows
 * rf = df - af and rr = (d - df) - ar.  Every difference stops at 0 and every cell at 2^32 - 1. */
int slh_format_vcf_sb_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const uint32_t *site_fwd, const slh_genotype *site_gts,
                           uint64_t sites, const slh_event *events, const uint32_t *anchor_rows, const uint32_t *anchor_fwd,
                           const slh_genotype *event_gts, const uint8_t *called, uint64_t num_events, int fs_filter);
/* -wq: the header of -vcf -gt (sb: of -sb, with fs_filter) with ##FORMAT=<ID=ADQ,Number=R,...> behind its FORMAT
 * lines, and the lines of slh_format_vcf_gt_rows (sb: of slh_format_vcf_sb_rows), each with one more sample value ADQ: on an SNV
 * line the quality sums of the reference and of each ALT letter in AD's order, from site_qsums (four per site: the A C G T
 * columns of the quality accumulator), on an indel line a dot.  site_fwd and anchor_fwd are looked at with sb only. */
int slh_format_vcf_wq_header(slh_buffer *buf, const slh_record *refs, int num_refs, int sb, int fs_filter);
int slh_format_vcf_wq_rows(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t record_size, const char *text,
                           const uint64_t *site_pos, const uint32_t *site_counts, const uint32_t *site_fwd, const uint32_t *site_qsums,
                           const slh_genotype *site_gts, uint64_t sites, const slh_event *events, const uint32_t *anchor_rows,
                           const uint32_t *anchor_fwd, const slh_genotype *event_gts, const uint8_t *called, uint64_t num_events, int sb,
                           int fs_filter);
/* -cons: one FASTA record -- '>' and the record's name up to its first blank or tab, then `len` letters in lines of 60; a record
 * of no letters is its header line alone */
int slh_format_fasta_record(slh_buffer *buf, const char *record_name, const char *letters, uint64_t len);
/* -depth.  The runs of slamem_pileup_depth_runs_* (the same two words), and the run of a record that is not written yet. */
typedef struct {
    uint64_t pos, value;
} slh_depth_run;
typedef struct {
    uint64_t start, end, value; /* local to the record */
    int open;
} slh_depth_pending;
/* The bedGraph lines (name, start, end, value; 0-based, half-open, local to the record that starts at row record_start) of rows
 * [a, b) of a record, from the runs of a range that holds them (runs[0].pos <= a; run i ends where run i + 1 starts, the last one
 * behind b or at it): the runs clipped to [a, b).  The piece's last run stays in *pend, and the first run of the record's next
 * piece continues it when it has the same value and starts where it ended -- a run over the border of two ranges is one line;
 * slh_format_depth_flush writes it (at the record's end) and is harmless when nothing is open. */
int slh_format_depth_runs(slh_buffer *buf, const char *record_name, uint64_t record_start, uint64_t a, uint64_t b,
                          const slh_depth_run *runs, uint64_t num_runs, slh_depth_pending *pend);
int slh_format_depth_flush(slh_buffer *buf, const char *record_name, slh_depth_pending *pend);
/* -depth -win N: the lines of windows j0 .. j0 + k - 1 of a record of record_size rows (window j is rows [j N, (j + 1) N), the
 * last one shorter): name, start, end and the mean depth 100 * sum // rows as whole "." two digits.  sum_at_j0 is the sum of d
 * in front of window j0, cum[2 i] the sum in front of the end of window j0 + i (the pairs of slamem_pileup_depth_runs_*). */
int slh_format_depth_windows(slh_buffer *buf, const char *record_name, uint64_t record_size, uint64_t window, uint64_t j0,
                             uint64_t sum_at_j0, const uint64_t *cum, uint64_t k);
/* -depth: the line of a record for stderr: "> Depth of NAME: L positions, C covered (P %), mean depth M", P = 10000 * C // L and
 * M = 100 * sum // L printed as above (both 0.00 for a record of no rows) */
int slh_format_depth_summary(slh_buffer *buf, const char *record_name, uint64_t length, uint64_t covered, uint64_t sum);
/* -stats: the report of a table of SLH_STATS_WORDS counters (the sections of include/slamem_hip.h), tab-separated,
 * the first column a section tag; histogram rows whose counts are all zero are left out, and a last bin that takes every higher
 * value prints its number with a `+`:
 *   SN name value     the sixteen totals, then clipped letters (counted letters - segment letters) and, per aligned letter
 *                     (matches + mismatches), mismatch rate and indel rate (insertions + deletions) as %.6f
 *   MQ q n            RL len n (511+)            NM edits n (127+)
 *   CY cycle aligned mismatches inserted deletions (511+)
 *   SU ref read n     BQ q aligned mismatches empirical, empirical = -10 log10((mismatches + 1) / (aligned + 2)) as %.2f
 *   IL len n (63+)    DL len n (63+)
 * Returns 0, or -1 when the file reports an error. */
#define SLH_STATS_WORDS 3112
int slh_write_stats(const uint64_t *table, FILE *f);
void slh_buffer_free(slh_buffer *b);
/* make room for `bytes` more characters in one step (slh_format_block grows the buffer by doubling otherwise) */
int slh_buffer_reserve(slh_buffer *b, size_t bytes);

/* The hidden utilities of the reference's command line: "-s <mems_file>" (SortMEMsFile, slamem.c:244-352) and
 * "-c <fasta_file>" (CleanFasta, slamem.c:455-523).  Messages go to log; the return value is the process status. */
int slh_sort_mems_file(const char *path, FILE *log);
int slh_clean_fasta(const char *path, FILE *log);

/* "-v <mems_file>" (CreateMemMapImage, slamem.c:354-452; graphics.c, bitmap.c): the picture of the MEMs of every query against
 * the one reference, written as <mems_file without extension>.bmp, the same bytes as the reference's.  seqs: the reference
 * record first, then every query record in loading order.  Returns the process status (0, or -1 after an error message). */
int slh_mem_map_image(const char *mems_path, const slh_record *seqs, int num_seqs, int num_refs, FILE *log);

/* (tests) an arbitrary 8-bit picture, rows top first, through the tool's file writer (palette of the tool; run-length coded, or
 * plain when that would not be shorter); 1 on success */
int slh_write_bmp8(const char *path, int width, int height, const uint8_t *rows_top_first);

/* number of progress dots the reference prints for a strand of this length (slamem.c:94,116-120) */
int slh_progress_dots(uint32_t textsize);

#ifdef __cplusplus
}
#endif
#endif
