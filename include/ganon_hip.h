/*
 * ganon_hip.h -- C ABI of libganon_hip.so: ganon's read-classification hot path on MI355X.
 *
 * This is the drop-in boundary.  It replaces exactly the two SeqAn3 call sites
 * of the reference's per-read loop and the per-read target selection that consumes them:
 *
 *   /root/reference/src/ganon-classify/GanonClassify.cpp:693-700
 *        hashes = seq | seqan3::views::minimiser_hash(k, w, adjust_seed(k))       -> gn_submit_batch
 *   /root/reference/src/ganon-classify/GanonClassify.cpp:514   (IBF)  agent.bulk_count(hashes)
 *   /root/reference/src/ganon-classify/GanonClassify.cpp:553   (HIBF) agent.bulk_count(hashes, thr)
 *   /root/reference/src/ganon-classify/GanonClassify.cpp:516-540 / :556-576  per-target sum, cap,
 *        cutoff test of select_matches                                              -> gn_fetch_batch
 *
 * Plain C: caller-owned host buffers, no exceptions, no globals besides a thread-local error
 * string.  Every function returns 0 on success or a negative GN_E* code; gn_last_error() gives
 * the message.  A gn_filter is immutable after upload and may be shared by any number of
 * gn_streams / host threads (mirrors "const member functions are thread-safe, one agent per
 * thread", hierarchical_interleaved_bloom_filter.hpp:79-83,501-504).  One gn_stream per host
 * worker thread; a stream owns a HIP stream, device batch buffers and pinned staging.
 *
 * There is no CPU fallback: every entry point fails (GN_ENODEV) when no HIP device is usable.
 */
#ifndef GANON_HIP_H
#define GANON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_OK 0
#define GN_EINVAL (-22)   /* bad argument */
#define GN_ENOMEM (-12)   /* host/device allocation failed */
#define GN_ENODEV (-19)   /* no usable HIP device / HIP runtime error */
#define GN_ERANGE (-34)   /* configuration outside what the kernels support (message says which) */
#define GN_EOVERFLOW (-75) /* caller's match buffer too small; *n_matches holds the needed size */

typedef struct gn_filter gn_filter;
typedef struct gn_stream gn_stream;

/* One flat interleaved Bloom filter as laid out by seqan3::interleaved_bloom_filter<uncompressed>
 * (the .ibf payload verbatim): word(row r, batch b) = rows[r*bin_words + b],
 * bit j of that word <-> bin 64*b + j. */
typedef struct
{
    const uint64_t* rows;      /* host pointer, bin_size*bin_words words; NULL = allocate zero-filled on device */
    uint64_t        bin_size;  /* S: rows (bin_size_, the number of bits of one Bloom filter) */
    uint64_t        bin_words; /* W = ceil(bins/64) */
    uint64_t        bins;      /* B: bin_count() */
    uint32_t        hash_funs; /* h <= 5 */
    uint32_t        hash_shift; /* countl_zero(bin_size) */
} gn_ibf_desc;

/* sparse result of select_matches for one (read, target): count already summed over the target's
 * bins and capped at n_hashes (GanonClassify.cpp:519-526 / :561-564), and >= the read's cutoff. */
typedef struct
{
    uint32_t read;   /* index in the batch */
    uint32_t target; /* caller's target id (IBF: bin2target[], HIBF: user bin index) */
    uint32_t count;
} gn_match;

/* per-read status written by gn_fetch_batch (GanonClassify.cpp:690,706) */
#define GN_READ_OK 0
#define GN_READ_SMALL 1 /* len(read1) < window_size: skipped, regardless of the mate (:690,743-747) */
#define GN_READ_BIG 2   /* more than 65535 minimisers: skipped (:674,706,737-741) */

/* device timings of the last gn_stream_classify, measured with hipEvents on the stream's HIP stream */
typedef struct
{
    float    ms_minimiser; /* slot scan + minimiser kernels (side stream; overlaps the count kernels of earlier chunks) */
    float    ms_count;     /* first IBF/HIBF count+select kernel start -> last one's end (main stream) */
    float    ms_total;     /* first kernel start -> last kernel end */
    uint64_t n_hashes;     /* minimisers of the batch (sum over reads that were counted) */
    uint64_t algo_bytes;   /* algorithmic row bytes: sum n*h*W*8 over every IBF visited */
    uint64_t n_matches;
    uint32_t n_count_launches; /* count/select launches of the batch (chunks of the minimiser||count pipeline); ms_count spans all */
    uint64_t fetched_bytes;    /* row bytes actually requested: algo_bytes minus the rows skipped by the exact early exit
                                  of reads that can no longer reach their cutoff (flat IBF fast path) */
    float    ms_compact;       /* 0, or the contiguous copy of a segmented result that a consumer asked for after the batch (a flat IBF with
                                  one unit per read leaves a read's matches where the count kernel wrote them; gn_fetch_batch(matches),
                                  gn_stream_device_matches and the merges make the copy on demand): not part of ms_total */
} gn_timings;

int         gn_device_count(int* n);
const char* gn_last_error(void);
/* The constants of seqan3's hash_and_fit this library was BUILT with (include/ganon_ibf_hash.h: five seeds, the multiplier), so that a
 * caller or a test can compare them with its own; needs no device.  Replaces nothing in the reference: the numbers live inside SeqAn3
 * (GanonClassify.cpp:514 -> bulk_count -> hash_and_fit). */
int         gn_ibf_hash_constants(uint64_t seeds[5], uint64_t* multiplier);

/* ---- filters ------------------------------------------------------------------------------- */

/* Flat IBF.  bin2target[b] (b < bins) = caller's target id of technical bin b, or 0xFFFFFFFF for
 * bins that belong to no target (replaces Filter::map, GanonClassify.cpp:279-287,1021-1025);
 * target ids must be < n_targets.  A target may own any set of bins (split bins, :516-523).
 * bin2target == NULL makes a STORAGE-ONLY filter (the builder's use): rows can be written, hashes inserted, rows read
 * back, but no stream can be created on it -- and the bin-count limit of the classify kernels does not apply. */
int gn_filter_upload_ibf(int device, const gn_ibf_desc* ibf, const uint32_t* bin2target, uint32_t n_targets,
                         gn_filter** out);

/* HIBF (raptor 3.0.1 layout, hierarchical_interleaved_bloom_filter.hpp:124-136,188):
 * next_ibf_id[i][b] and bin2userbin[i][b] (-1 = merged bin) for every bin b < ibfs[i].bins.
 * Reported target id = user bin index (ibf_bin_to_filename_position).
 * A bin with bin2userbin == -1 AND next_ibf_id == -1 is ABSENT: it belongs to another part of an HIBF that is spread over
 * several devices by subtree (below: gn_gather_create_merged).  It is never reported and never descended into, and
 * gn_filter_finalize clears its bits in every row, so that rows streamed in with gn_filter_write_rows(word_lo) may carry
 * the neighbours' bins of a boundary word.  (The reference has no such bins: it holds the whole tree in host memory.) */
int gn_filter_upload_hibf(int device, uint32_t n_ibf, const gn_ibf_desc* ibfs, const int64_t* const* next_ibf_id,
                          const int64_t* const* bin2userbin, uint64_t n_user_bins, gn_filter** out);

/* OR minimiser hashes into technical bins of a flat IBF on the device (interleaved_bloom_filter::emplace,
 * call site src/ganon-build/GanonBuild.cpp:694).  n (hash, bin) pairs in host memory. */
int gn_filter_emplace(gn_filter* f, const uint64_t* hashes, const uint32_t* bins, uint64_t n);

/* Same for IBF `ibf_idx` of an HIBF (ibf_idx = 0 for a flat filter). */
int gn_filter_emplace_ibf(gn_filter* f, uint32_t ibf_idx, const uint64_t* hashes, const uint32_t* bins, uint64_t n);

/* copy rows [row_begin, row_begin+n_rows) of IBF `ibf_idx` back to the host (tests / sampling parity) */
int gn_filter_download_rows(const gn_filter* f, uint32_t ibf_idx, uint64_t row_begin, uint64_t n_rows, uint64_t* out);
/* gather rows row_idx[0..n) of IBF `ibf_idx` (bin_words words each) into out[n*bin_words]: the sampling parity
 * checks on filters too large to download (BASELINE configs 4/5) fetch only the rows their sample touches */
int gn_filter_download_row_list(const gn_filter* f, uint32_t ibf_idx, const uint64_t* row_idx, uint64_t n, uint64_t* out);

/* ---- streaming load (filter loaders, /root/reference/src/ganon-classify/GanonClassify.cpp:949-986 load_filter:
 * the reference deserialises the whole sdsl bit_vector into host memory; here the payload goes to HBM chunk by chunk).
 * gn_filter_upload_ibf/hibf with rows == NULL allocate a zero-filled matrix; gn_filter_write_rows then copies
 * rows [row_begin, row_begin+n_rows) of IBF `ibf_idx` from a host chunk whose rows are src_row_words wide, keeping
 * words [word_lo, word_lo + bin_words) of every row (word_lo > 0 / src_row_words > bin_words = one column slice of
 * a bin-range partitioned filter).  With `src` from gn_pinned_alloc the copy is asynchronous on the
 * filter's load stream: the caller may refill the OTHER staging buffer meanwhile and must call
 * gn_filter_write_sync before reusing `src`.  gn_filter_finalize clears the padding bins and waits. */
int gn_pinned_alloc(size_t bytes, void** out);
int gn_pinned_free(void* p);
int gn_filter_write_rows(gn_filter* f, uint32_t ibf_idx, uint64_t row_begin, uint64_t n_rows, const uint64_t* src,
                         uint64_t src_row_words, uint64_t word_lo);
int gn_filter_write_sync(gn_filter* f);
int gn_filter_finalize(gn_filter* f);

/* Synthetic content for benchmarks / full-size parity tests (SURVEY 8d "generated on device for >= 8 GiB"):
 *   word(r, j) = AND_{a < and_words} mix64(mix64(seed + a) + (r * row_words_total + word_lo + j) * 0x9E3779B97F4A7C15)
 * with mix64 = the splitmix64 finaliser, i.e. iid Bernoulli(2^-and_words) bits that depend only on the GLOBAL word
 * position -- a column slice (word_lo, row_words_total of the whole filter) holds exactly the bits the unsliced
 * filter has there.  Padding bins are cleared.  Not part of the reference's interface.
 * and_words = GN_FILL_3_OF_8: word = m0 & (m1 | m2) with m_a = the mixes above, density 3/8 -- what a Bloom filter built for a
 * false-positive rate of 0.05 with three hash functions looks like (0.375^3 = 0.053).
 * and_words = GN_FILL_3_OF_16: word = m0 & m1 & (m2 | m3), density 3/16 -- an HIBF at the reference's defaults: `ganon build
 * --filter-type hibf` passes --max-fp 0.001 and --hash-functions 4 to raptor (/root/reference/src/ganon/config.py:140-143,
 * 1258-1260, build_update.py:487-489); 0.1875^4 = 0.0012. */
#define GN_FILL_3_OF_8 0x38u
#define GN_FILL_3_OF_16 0x3Fu
int gn_filter_fill_random(gn_filter* f, uint32_t ibf_idx, uint64_t seed, uint32_t and_words, uint64_t word_lo,
                          uint64_t row_words_total);

int gn_filter_info(const gn_filter* f, int* is_hibf, uint32_t* n_ibf, uint64_t* n_targets, uint64_t* device_bytes);
int gn_filter_free(gn_filter* f);

/* ---- streams ------------------------------------------------------------------------------- */

/* max_matches = capacity of the device match buffer; 0 picks max_reads*4 (it grows on demand). */
int gn_stream_create(gn_filter* f, uint32_t max_reads, uint64_t max_bases, uint64_t max_matches, gn_stream** out);
int gn_stream_destroy(gn_stream* s);

/* Batch layout: `bases` holds ASCII nucleotides (dna15 alphabet, any case; converted to dna4 ranks on
 * the device exactly like seqan3::dna4).  Read i = bases[off1[i] .. off1[i+1]) and, if
 * off2 != NULL, its mate = bases[off2[i] .. off2[i+1]).  off1/off2 have n_reads+1 entries.
 * k, w: minimiser shape; the seed is adjust_seed(k) (src/utils/include/utils/adjust_seed.hpp:33-37).
 * rel_cutoff: per-read cutoff T = max(1, ceil(n_hashes*rel_cutoff)) computed in IEEE double on the
 * device, bit-identical to GanonClassify.cpp:492-495,720-724. */

/* H2D only (asynchronous on the stream). */
int gn_stream_upload_reads(gn_stream* s, const uint8_t* bases, uint64_t n_bases, const uint64_t* off1,
                           const uint64_t* off2, uint32_t n_reads);
/* Minimiser hashes only (asynchronous): the build-side use of the same view
 * (/root/reference/src/ganon-build/GanonBuild.cpp:198-200,236); results via gn_stream_fetch_hashes. */
int gn_stream_minimisers(gn_stream* s, uint32_t k, uint32_t w);
/* Kernels only, on the reads currently resident in the stream (asynchronous). */
int gn_stream_classify(gn_stream* s, uint32_t k, uint32_t w, double rel_cutoff);
/* upload + classify (asynchronous) -- the call the reference's loop body maps to */
int gn_submit_batch(gn_stream* s, const uint8_t* bases, uint64_t n_bases, const uint64_t* off1, const uint64_t* off2,
                    uint32_t n_reads, uint32_t k, uint32_t w, double rel_cutoff);
/* Several filters on ONE device see the same batch -- the filters of a hierarchy level (same k, w: GanonClassify.cpp:1479-1494), or
 * the column parts of a wide / partitioned filter: the reference hashes a read once and hands the hashes to every filter's agent
 * (:693-735).  gn_stream_classify_shared counts the batch that is resident in `source` (uploaded and hashed there by
 * gn_submit_batch / gn_stream_classify / gn_stream_minimisers) against the filter of `s` as well, without uploading or hashing
 * again (asynchronous; k, w are the source's).  Everything that follows -- gn_fetch_batch, the pre-pass, gn_gather -- works on `s`
 * as after gn_stream_classify.  The caller fetches (or syncs) every sharing stream before it puts the next batch into `source`. */
int gn_stream_classify_shared(gn_stream* s, gn_stream* source, double rel_cutoff);

/* Reads as they lie in the file: uncompressed four-line FASTQ text instead of packed bases.  Replaces, for such input, the record
 * parsing of the reference's input side (seqan3::sequence_file_input in parse_reads, GanonClassify.cpp:1220-1287) together with
 * gn_stream_upload_reads: `text` (n_bytes <= the stream's max_bases, first byte = first byte of a record) is copied to the device
 * and the records are found there.  A record is taken when its four lines are  @id / letters / +... / quality  with as many
 * quality characters as letters and dna15 letters only (a '\r' before the '\n' of the letters line does not count); the first
 * record that is not -- or the end of the text inside a record, or the stream's max_reads -- ends the batch.  Asynchronous.
 *   gn_stream_fastq_index   waits for the tokeniser: the batch's reads (records before the first one not taken), their bases,
 *                           and parsed_bytes = offset of the first byte that is not part of them (== n_bytes: all of the text).
 *                           From here on the stream holds the batch as after gn_stream_upload_reads (single-end):
 *                           gn_stream_classify / gn_stream_minimisers / gn_fetch_batch apply, read i = record i.
 *   gn_stream_fastq_keep    the caller takes fewer records than were found (before gn_stream_classify)
 *   gn_stream_fastq_records per read: offset of its record ('@'), of its first letter, and its number of letters, in `text`
 *                           (any may be NULL; waits for the stream) -- ids and letters stay where they are, in the caller's text */
int gn_stream_upload_fastq(gn_stream* s, const uint8_t* text, uint64_t n_bytes);
/* The same for either text format.  GN_TEXT_FASTA: records of two lines,  >id / letters  -- every record's letters on one line and
 * the next line a '>' (or the end of the text); a wrapped sequence, a blank line or a ';' header ends the batch before its record,
 * like a FASTQ record the four-line rule does not cover.  gn_stream_fastq_index / _keep / _records apply unchanged (rec_at = the '>'). */
#define GN_TEXT_FASTQ 0
#define GN_TEXT_FASTA 1
int gn_stream_upload_text(gn_stream* s, const uint8_t* text, uint64_t n_bytes, int format);
/* Paired input as text: a piece of each mate file, both beginning with a record and holding the SAME records by number (the caller
 * cuts the second file where the first file's piece ends, counted in records: parse_reads takes file 2 with take(n_reads),
 * GanonClassify.cpp:1240-1252).  Both texts are tokenised; the batch is the pairs BOTH hold before the first group of lines
 * that is no record in either: read i = record i of text1 with record i of text2 as its mate (its id is text1's, :1244).
 * n_bytes1 rounded up to 16, plus n_bytes2, must fit the stream's max_bases.
 *   gn_stream_text_pair_index     waits; the pairs taken and the bytes of each text they cover (== n_bytes: all of it)
 *   gn_stream_fastq_keep / gn_stream_fastq_records (text1's records) apply; gn_stream_text_pair_records2 = the mates' in text2 */
int gn_stream_upload_text_pair(gn_stream* s, const uint8_t* text1, uint64_t n_bytes1, const uint8_t* text2, uint64_t n_bytes2, int format);
/* The same for a text that is in device memory already (of device src_device; the stream's own or a peer): the piece of a gzip file
 * that gn_inflate_step left there (gn_inflate_text_device + the offsets of gn_inflate_cuts).  The caller does not hold the text, so
 *   gn_stream_fastq_headers   (after gn_stream_fastq_index / _keep) copies the batch's header lines -- '@' or '>' to the newline, both
 *                             included -- back to back to dst, record i's at hdr_off[i] (hdr_off has n_reads + 1 entries; *n_bytes =
 *                             hdr_off[n_reads]; GN_EOVERFLOW with *n_bytes set when cap is too small): ids as in parse_reads
 *                             (GanonClassify.cpp:1244,1262: the whole header line) without the text crossing the link */
int gn_stream_upload_text_device(gn_stream* s, const uint8_t* d_text, uint64_t n_bytes, int format, int src_device);
/* both mate files' pieces in device memory (as gn_stream_upload_text_pair otherwise) */
int gn_stream_upload_text_pair_device(gn_stream* s, const uint8_t* d_text1, uint64_t n_bytes1, const uint8_t* d_text2, uint64_t n_bytes2, int format,
                                      int src_device);
/* ... the two pieces on two devices (the mate files of a pair inflated by different inflaters, gn_inflate_set_turns) */
int gn_stream_upload_text_pair_devices(gn_stream* s, const uint8_t* d_text1, uint64_t n_bytes1, int src_device1, const uint8_t* d_text2, uint64_t n_bytes2,
                                       int src_device2, int format);
int gn_stream_fastq_headers(gn_stream* s, uint8_t* dst, uint64_t cap, uint32_t* hdr_off, uint64_t* n_bytes);
/* The resident batch's letters as the kernels see them (ASCII, mate-1 block then mate-2 block: the layout of gn_stream_upload_reads) with
 * off1 / off2 (n_reads + 1 entries each; off2 only for pairs): for a caller that classified a text it does not hold and needs the letters
 * after all -- reads left unclassified go on to the next hierarchy level (GanonClassify.cpp:811-820).  *n_bytes = bytes copied
 * (GN_EOVERFLOW with *n_bytes set when cap is too small). */
int gn_stream_fetch_letters(gn_stream* s, uint8_t* bases, uint64_t cap, uint64_t* off1, uint64_t* off2, uint64_t* n_bytes);
int gn_stream_text_pair_index(gn_stream* s, uint32_t* n_reads, uint64_t* parsed_bytes1, uint64_t* parsed_bytes2);
int gn_stream_text_pair_records2(gn_stream* s, uint32_t* rec_at, uint32_t* seq_at, uint32_t* seq_len);
int gn_stream_fastq_index(gn_stream* s, uint32_t* n_reads, uint64_t* n_bases, uint64_t* parsed_bytes);
int gn_stream_fastq_keep(gn_stream* s, uint32_t n_reads);
int gn_stream_fastq_records(gn_stream* s, uint32_t* rec_at, uint32_t* seq_at, uint32_t* seq_len);
/* A genome as it comes: wrapped, multi-record FASTA text, tokenised on the device for the builder (gn_genome.hip).  `text` is host
 * memory, n_bytes <= the stream's max_bases, and its first byte is the first byte of a line.  Asynchronous; gn_stream_genome_index waits.
 * The record rules are those of the host's sequential reader: a line whose first byte is '>' or ';' begins a record and none of its
 * bytes is a letter; blank lines are ignored everywhere; in any other line isspace bytes and the digits are ignored, the dna15 letters
 * ABCDGHKMNRSTUVWY (either case) are kept and any other byte gives status GN_GENOME_BAD_LETTER with bad_at = its offset; a non-blank
 * line before the first header (without GN_GENOME_CONTINUES) gives GN_GENOME_NO_HEADER.  The text may end without a newline.
 * A record is kept when it has >= min_length letters; a kept record with >= w letters is cut into pieces that begin every `stride`
 * letters while a whole window fits, each of min(letters left, stride + w - 1) letters, written back to back into the stream's base
 * buffer with off1: after gn_stream_genome_index the stream holds the batch as after gn_stream_upload_reads (read i = piece i), and
 * gn_stream_minimisers, gn_stream_distinct_hashes and gn_stream_distinct_hashes_packed apply unchanged (with no piece there is
 * nothing to hash).  Whole records are taken while their number and their pieces are <= max_reads and their bytes <= max_bases:
 * parsed_bytes = offset of the first record not taken (== n_bytes: all were); a first record that alone is too large is GN_ERANGE.
 *   GN_GENOME_OPEN_END   the text ends inside its last record: that record is hashed whatever its length so far (state 3),
 *                        open_letters = its letters including what earlier texts carried, and the stream keeps its last
 *                        min(letters, w - 1) letters and its length on the device
 *   GN_GENOME_CONTINUES  text[0] continues the record the previous text on this stream left open: the carried letters are the
 *                        head of its first piece, so every window across the cut is hashed exactly once.  It is record 0, with
 *                        rec_at 0 and rec_letters counting the carried letters as well
 *   gn_stream_genome_records  per record (any may be NULL): offset of its header in the text, its letters, and its state --
 *                        0 hashed, 1 below min_length, 2 kept but with fewer than w letters (not hashed here: the caller takes the
 *                        letters from its own text, rec_at[r] up to the next record, and hashes them as a whole), 3 open at the end */
#define GN_GENOME_CONTINUES 1u  /* text[0] continues the record the previous call on this stream left open */
#define GN_GENOME_OPEN_END  2u  /* the text ends inside its last record (the caller cut at a newline, not at a header) */
#define GN_GENOME_BAD_LETTER 1
#define GN_GENOME_NO_HEADER 2
int gn_stream_upload_genome_text(gn_stream* s, const uint8_t* text, uint64_t n_bytes, uint32_t w, uint32_t stride, uint64_t min_length, uint32_t flags);
int gn_stream_genome_index(gn_stream* s, uint32_t* n_records, uint32_t* n_pieces, uint64_t* n_bases, uint64_t* parsed_bytes, int* status,
                           uint64_t* bad_at, uint64_t* open_letters);
int gn_stream_genome_records(gn_stream* s, uint64_t* rec_at, uint64_t* rec_letters, uint8_t* rec_state);
int gn_stream_sync(gn_stream* s);

/* Wait for the batch and copy results out.  n_hashes[n_reads], status[n_reads], match_off[n_reads+1]
 * (any may be NULL); matches[cap] receives the matches grouped by read (ascending read, then ascending
 * target).  Returns GN_EOVERFLOW with *n_matches = required capacity if cap is too small. */
int gn_fetch_batch(gn_stream* s, uint32_t* n_hashes, uint8_t* status, uint64_t* match_off, gn_match* matches,
                   uint64_t cap, uint64_t* n_matches);

/* Reads with more than 65535 minimisers.  By default they come back with status GN_READ_BIG and no matches, like the
 * reference's default build (TIntCount = uint16_t, GanonClassify.cpp:45-49,674).  on != 0 gives what the reference does when
 * compiled with -DLONGREADS (uint32 counters): such reads are counted with 32-bit counters (flat IBF: by a kernel of their
 * own; HIBF: by the LDS-counter level kernel), come back with status GN_READ_OK, and their match counts may exceed 65535.
 * For an HIBF the option also switches the 16-bit wrap of the per-user-bin sums off for every read, as the uint32 build does
 * (hibf.hpp:438,442: value_t). */
int gn_stream_set_long_reads(gn_stream* s, int on);

/* Optional device-side pre-pass of filter_matches (/root/reference/src/ganon-classify/GanonClassify.cpp:579-613 with the
 * threshold of :755-761) on every following batch of this stream: with max/min = the read's largest/smallest match count
 * (min starts at n_hashes, :704), matches below max - ceil((max-min)*rel_filter) are dropped (exact), and, if fpr_query < 1,
 * matches whose q = 1 - BinomCDF(count; n_hashes, target_fpr[target]) is above fpr_query BY A SAFE MARGIN are dropped too
 * (q > fpr_query*1.001 + 1e-9; the caller applies the exact rule to what is left, so the final result is the reference's).
 * A surviving match whose q is below fpr_query by the same margin (q < fpr_query*0.999 - 1e-9) comes back with
 * GN_MATCH_FPR_OK set in its count: the caller may skip its own evaluation for it (mask the bit off to get the count).
 * gn_fetch_batch / gn_stream_device_matches then return the survivors only.  Use it only where this filter sees all of a
 * read's matches (one filter per hierarchy level, filter not cut into column parts).  target_fpr: n_targets doubles
 * (flat IBF) / n_user_bins doubles (HIBF); may be NULL when fpr_query >= 1.  pf == NULL switches the pass off. */
#define GN_MATCH_FPR_OK 0x80000000u
typedef struct gn_postfilter
{
    double        rel_filter;
    double        fpr_query;
    const double* target_fpr;
    int           joint; /* 0: the pass runs with every batch.  1 / 2: one of several filters of a hierarchy level (see below) */
    const uint32_t* target_gid; /* joint == 2: level-wide id (< 2^28) of every target of this filter (same size as target_fpr) */
} gn_postfilter;
int gn_stream_set_postfilter(gn_stream* s, const gn_postfilter* pf);
/* A hierarchy level with several filters: the reference merges their matches before it thresholds (:716-735,755-761), so a
 * read's max/min are the level's.  If the filters' targets are DISJOINT (no target can be reported by two of them) the
 * pre-pass still works per filter: submit the same batch to one stream per filter (same device, post-filters set with
 * joint = 1), then call this once: it finds every stream's max/min per read, combines them, and applies the rules to every
 * stream with the level's values.  Afterwards gn_fetch_batch / gn_fetch_postfilter work per stream as above (max_count is the
 * level's maximum on every stream).
 * If the filters SHARE targets, set joint = 2 and target_gid on every stream (an id per target name, the same id for the same
 * name in every filter; a filter names a target once): the call then replays the reference's merge per read (:531-537: a
 * target keeps its largest count, the entry of the earliest stream in `streams` on ties; max/min follow the entries that got
 * in), keeps only the winning entry of every target -- on the stream of the filter that reported it -- and applies the rules
 * to the winners.  Reads with more than 4096 matches over all streams are left untouched and come back with bit 31 of
 * max_count set on every stream: the caller merges and thresholds those itself.  The dropped-match totals of a merging pass
 * are reported on streams[0]. */
int gn_streams_postfilter_joint(gn_stream* const* streams, uint32_t n_streams);
/* The streams of a joint pass over DISJOINT targets may sit on several devices -- the column parts of a bin-range
 * partitioned filter (below): every device combines its streams' max/min per read, the devices exchange those two arrays
 * (8 bytes per read and pair of devices, hipMemcpyPeerAsync over xGMI), and every stream applies the rules with the level's
 * values.  Up to 16 streams per device and 16 devices.  A merging pass (joint = 2) needs all its streams on one device. */
/* after a batch with the pass on: per read the largest match count BEFORE filtering (0 = the read had no match; the
 * reference's max_count_read, :753,776,806), and how many matches each rule dropped in this batch */
int gn_fetch_postfilter(gn_stream* s, uint32_t* max_count, uint64_t* dropped_rel_filter, uint64_t* dropped_fpr_query);

/* Device-resident view of the same result for callers that forward it without a host round trip (the sparse-match
 * exchange of a bin-range partitioned filter sends it over RCCL straight from HBM): waits for the batch,
 * then *d_matches points to n_matches records in DEVICE memory, grouped by read (ascending read, then target).
 * The memory belongs to the stream and is valid until its next submit/classify/destroy. */
int gn_stream_device_matches(gn_stream* s, const gn_match** d_matches, uint64_t* n_matches);

/* ---- bin-range partitioned flat IBF (BASELINE config 5) ------------------------------------------------
 * The reference loads a filter of any size into host memory (/root/reference/src/ganon-classify/GanonClassify.cpp:949-986,
 * 1007-1039) and one bulk_count sees all of its bins (:514).  A filter larger than one GPU's HBM is cut by technical-bin
 * range, at boundaries between targets, into column parts: part g is a flat IBF of its own (gn_filter_upload_ibf with the
 * part's bins and a part-local target numbering, rows streamed with gn_filter_write_rows(word_lo = the part's first word)),
 * created on whichever device has room.  Every part classifies every batch (one gn_stream per part, same reads); the cutoff
 * and the per-target sum of :516-527 are complete inside a part because a target's bins never straddle a cut.
 * gn_gather puts a read's matches back together on the batch's OWNER device: the parts' grouped matches and per-read
 * offsets are copied device to device (hipMemcpyPeerAsync: xGMI, not the host) and one kernel concatenates them per read in
 * part order -- ascending target, since targets ascend with the bins -- translating part-local target ids through
 * target_map[i] (n_map[i] entries; NULL = ids are the caller's already).  Parts that live on the owner device are read in
 * place.  With a filter_matches pre-pass set on the parts' streams (joint = 1), call gn_streams_postfilter_joint over them
 * first: then only survivors travel.  The result is what gn_fetch_batch would return for the unpartitioned filter. */
typedef struct gn_gather gn_gather;
int gn_gather_create(int device, uint32_t n_parts, const uint32_t* const* target_map, const uint32_t* n_map, gn_gather** out);
/* The same for an HIBF that does not fit one device and is spread BY SUBTREE: the reference's counting agent walks one tree in
 * host memory (hierarchical_interleaved_bloom_filter.hpp:432-460) and select_matches(THIBF) reads the counts by user bin
 * (GanonClassify.cpp:543-577).  A technical bin of the root is reported or descended into on its own count alone and everything
 * below a merged bin is reached through it only, so the root's bins -- each with its whole subtree -- are dealt to the devices;
 * every part is an HIBF of its own (gn_filter_upload_hibf with absent bins, a root of words [word_lo, word_hi) of the root's
 * rows, user bins renumbered densely in ascending global id).  User bins are numbered by file position and laid out by size,
 * so the parts' ids interleave: this gather MERGES a read's segments by translated id instead of putting them behind each
 * other.  Preconditions: every target_map[i] is strictly increasing (NULL = the identity), every part's segment of a read
 * ascends in part-local id (gn_fetch_batch order), translated ids of different parts are disjoint (equal ids: lower part
 * first).  Result, per read: the union of the parts' records in ascending translated id -- for an HIBF what gn_fetch_batch
 * of the unpartitioned filter gives.  gn_gather_run accepts streams on HIBFs only from a gather created here. */
int gn_gather_create_merged(int device, uint32_t n_parts, const uint32_t* const* target_map, const uint32_t* n_map, gn_gather** out);
/* streams[i] = part i's stream, all holding the same submitted batch (gn_submit_batch / gn_stream_classify) */
int gn_gather_run(gn_gather* g, gn_stream* const* streams, uint32_t n_streams);
/* The same over parts that are plain DEVICE buffers on the gather's device -- the receive buffers of a multi-process job
 * (one process per GPU, the parts' records arrive over RCCL: ganon_amd/partition.py).  d_off[i]: n_reads+1 offsets of part
 * i, of any origin (read r of part i = d_matches[i][d_off[i][r] - d_off[i][0] .. d_off[i][r+1] - d_off[i][0])), n_matches[i]
 * its record count.  The caller's own stream must be done with the buffers. */
int gn_gather_run_buffers(gn_gather* g, const uint64_t* const* d_off, const gn_match* const* d_matches, const uint64_t* n_matches,
                          uint32_t n_parts, uint32_t n_reads);
/* per-read offsets (n_reads+1, device memory) that go with gn_stream_device_matches; valid as long as those */
int gn_stream_device_offsets(gn_stream* s, const uint64_t** d_match_off);
/* match_off[n_reads+1], matches[cap] grouped by read (ascending read, then ascending target); either may be NULL */
int gn_gather_fetch(gn_gather* g, uint64_t* match_off, gn_match* matches, uint64_t cap, uint64_t* n_matches);
/* device-resident view (valid until the next gn_gather_run) and the bytes the last run moved between devices */
int gn_gather_device_matches(gn_gather* g, const gn_match** d_matches, const uint64_t** d_match_off, uint64_t* n_matches,
                             uint64_t* peer_bytes);
int gn_gather_destroy(gn_gather* g);
/* What gn_gather did between devices so far, per ordered pair (dst = the gathering device): *state = 0 never needed, 1 peer
 * access enabled (hipDeviceEnablePeerAccess: direct copies over the xGMI link of the pair), 2 refused or not available (the
 * runtime stages the copy); *bytes = what travelled src -> dst.  `ganon-classify --verbose` prints it per pair. */
int gn_peer_stats(int dst, int src, int* state, uint64_t* bytes);

/* Switches (test and measurement hook; no counterpart in the reference).  The library reads its environment in ONE place:
 * $GANON_HIP_ABLATE, a comma list parsed once when the library is loaded (and, there too, $GANON_HIP_STREAM_ROWS_MIN_BYTES:
 * gn_filter_set_stream_rows_min_bytes).  gn_ablate() replaces that list in-process so a
 * test can cross-check a fast path against the path it replaces (NULL or "" = the product path).  Call it only while no
 * launch is in flight.  Names that switch a path OFF: early_exit row_screen lean_screen stray_masks stream_rows cand_select csr_identity uniform_select run_select
 * max_first const_nb split_kernel predrop deferred_grids hibf_reg hibf_pack hibf_one_pack; test set-ups:
 * pinned_malloc gather_copy joint_apart inflate_ahead on_demand hibf_dense_rows chunk=N hibf_pair_limit=N; runtime: sync=spin|yield|block debug; measurement with WRONG results: fake_count (flat IBF: the count +
 * select kernels are not run, every second read gets one made-up match -- what is left is what the host around the device sustains).  Unknown name -> GN_EINVAL and
 * the previous list stays. */
int gn_ablate(const char* list);
/* free / total memory of a device: the host decides with it whether a filter is replicated or partitioned */
int gn_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);
/* Words from one row to the next that gn_filter_upload_hibf gives an IBF of `bin_words` = ceil(bins / 64) words a row on the
 * device: rows are padded to whole 128-byte lines there (3 -> 4, 5..8 -> 8, 9..16 -> 16 words, multiples of 16 beyond), so that
 * no row request moves two lines.  An IBF of bin_size rows takes bin_size * this * 8 bytes -- what the host's placement must
 * count instead of the file's payload.  Everything the ABI takes or returns stays bin_words words a row.  (No counterpart in the
 * reference: /root/reference/src/ganon-classify/GanonClassify.cpp:949-986 reads the filter into host memory as it is.) */
uint64_t gn_hibf_row_stride_words(uint64_t bin_words);

/* ---- reassign: the EM over a classification's .all ---------------------------------------------------
 * `ganon classify` runs this after the binary by default (/root/reference/src/ganon/classify.py:76-88, --multiple-matches
 * em); the algorithm is /root/reference/src/ganon/reassign.py:96-145 with get_top_match :226-241.
 * The table is CSR over reads: off[n_reads+1] into target[n_entries]; a read's entries are in the order its lines appear in
 * the .all file, reads in first-appearance order, targets numbered 0..n_targets-1 by first appearance (:76-92) -- the
 * tie-break of get_top_match (first listed entry wins) and the left-to-right double sum of the convergence test depend
 * on exactly that order.  The table is copied to the device once and every iteration runs there.
 * gn_reassign_run: max_iter = 0 iterates until diff <= threshold (:141-145); diffs[i] = the i-th iteration's
 * sum |old prob - new prob| bit for bit as the reference computes it (gn_reassign_diffs copies the first `cap` of them).
 * gn_reassign_fetch (any pointer may be NULL): counts[t] = reassigned_matches of the LAST iteration (:113-121; the new .rep
 * holds counts[t] - unique[t] in its lca column, :189-219), unique[t] = reads listing t and nothing else, prob[t] after the
 * last update, choice[r] = index into target[] of the entry read r is given in the .one file (:153-181).
 * PRECONDITION (since round 5): every read has at least one entry, off[r + 1] > off[r] -- the reference's table holds a read only once a
 * line of the .all file names it (:76-92); a CSR with an empty row is refused with GN_EINVAL (an empty row has no entry choice[r] could
 * index, and the .one writer would have nothing to print).  A caller that holds reads without matches drops them before the call. */
typedef struct gn_reassign gn_reassign;
int gn_reassign_create(int device, uint64_t n_reads, uint64_t n_entries, uint32_t n_targets, const uint64_t* off,
                       const uint32_t* target, gn_reassign** out);
int gn_reassign_run(gn_reassign* g, uint32_t max_iter, double threshold, uint32_t* iterations);
int gn_reassign_diffs(const gn_reassign* g, double* diffs, uint32_t cap);
int gn_reassign_fetch(gn_reassign* g, uint64_t* counts, uint64_t* unique, double* prob, uint64_t* choice);
/* reads with one / several entries, reads long enough to take a wave of their own, device time of the last run (EM +
 * final choice) and the algorithmic bytes one iteration reads (8 per read, 4 per entry of a read with several + 4 for its last choice) */
int gn_reassign_info(const gn_reassign* g, uint64_t* n_unique_reads, uint64_t* n_multi_reads, uint64_t* n_wave_reads, float* ms_em,
                     uint64_t* bytes_per_iteration);
int gn_reassign_free(gn_reassign* g);

/* Build side (/root/reference/src/ganon-build/GanonBuild.cpp).
 * gn_stream_distinct_hashes: after gn_stream_minimisers, the SET of minimiser hashes of all sequences resident in the
 * stream, ascending -- what count_hashes collects per file in a robin_hood::unordered_set (:184-249; the set's own iteration
 * order is not reproducible here, ascending order is this library's definition).  out may be NULL to query *n_distinct.
 * A long sequence is passed as overlapping pieces (consecutive pieces share window_size-1 bases): every window lies in one
 * piece, so the set is the sequence's (emission order and duplicates differ, the set does not).
 * gn_filter_emplace_split: hash i of `hashes` is inserted into technical bin first_bin + i / hashes_per_bin -- a target's
 * run of bins with equal shares, create_bin_map_hash (:619-653) + build (:655-698). */
int gn_stream_distinct_hashes(gn_stream* s, uint64_t* out, uint64_t cap, uint64_t* n_distinct);
int gn_filter_emplace_split(gn_filter* f, const uint64_t* hashes, uint64_t n, uint32_t first_bin, uint64_t hashes_per_bin);
/* gn_filter_emplace_runs_window: the insert of build (/root/reference/src/ganon-build/GanonBuild.cpp:655-698) for a filter that is
 * built in slabs of rows.  `f` is a storage-only flat filter of n rows that stands for rows [row_begin, row_begin + n) of a filter of
 * total_rows rows (1 .. 2^32 - 1).  Run r is runs[r][0 .. run_sizes[r]) in host memory; hash i of it belongs to bin
 * first_bin[r] + i / hashes_per_bin[r], the rule of gn_filter_emplace_split.  For each of the filter's hash functions the row is that of
 * the WHOLE filter -- hash_and_fit with total_rows and countl_zero(total_rows), not with f's own -- and the bit is set at row
 * row - row_begin of f only when the row lies in the window; nothing else is touched.  With row_begin = 0 and total_rows = n the call
 * sets exactly the bits a loop of gn_filter_emplace_split over the runs sets.  All runs of a call go through two page-locked staging
 * chunks of chunk_hashes hashes (0: 1 Mi hashes, 8 MiB each; a run may be longer than a chunk), the upload of one under the kernel
 * of the one before, one launch per chunk; every bin a run can reach is checked before anything is launched. */
int gn_filter_emplace_runs_window(gn_filter* f, const uint64_t* const* runs, const uint64_t* run_sizes, const uint32_t* first_bin,
                                  const uint64_t* hashes_per_bin, uint32_t n_runs, uint64_t total_rows, uint64_t row_begin, uint64_t chunk_hashes);
/* Hash sets packed as deltas of fixed width (ganon_amd/csrc/gn_packed_set.h has the format, a host encoder and decoder).  A block holds
 * cnt hashes (1 .. 512), strictly ascending: `first` is the first, `width` the bit length of the largest difference of neighbours (0 for
 * one hash), and delta i-1 = v[i] - v[i-1] occupies bits [(i-1) * width, i * width) of the payload words from `word_at` on, LSB first,
 * across word boundaries; a block has ceil((cnt-1) * width / 64) words and its padding bits are zero.  A set is cut every 512 hashes.
 * gn_stream_distinct_hashes_packed: the set of gn_stream_distinct_hashes, packed on the device; only the packed bytes are copied.
 * With blocks and payload NULL the call answers *n_distinct, *n_blocks and *n_words alone; word_at counts from payload[0].  The result is
 * word for word what gn_packed_encode makes of the output of gn_stream_distinct_hashes.
 * gn_filter_emplace_packed_window: gn_filter_emplace_runs_window for packed runs.  Run r is blocks[r][0 .. n_blocks[r]) with word_at
 * counting from payload[r][0]; its hashes are those of its blocks behind each other (a short block may lie in the middle: a run is a
 * target's files' sets), hash i of them belongs to bin first_bin[r] + i / hashes_per_bin[r].  The same filter, window, checks and bits as
 * gn_filter_emplace_runs_window; the two staging chunks hold chunk_words payload words (0: 1 Mi words; at least the 511 words a block can
 * have) and the tables of their blocks. */
typedef struct gn_packed_block
{
    uint64_t first, word_at;
    uint32_t cnt, width;
} gn_packed_block;
int gn_stream_distinct_hashes_packed(gn_stream* s, gn_packed_block* blocks, uint64_t cap_blocks, uint64_t* payload, uint64_t cap_words,
                                     uint64_t* n_distinct, uint64_t* n_blocks, uint64_t* n_words);
int gn_filter_emplace_packed_window(gn_filter* f, const gn_packed_block* const* blocks, const uint64_t* n_blocks, const uint64_t* const* payload,
                                    const uint32_t* first_bin, const uint64_t* hashes_per_bin, uint32_t n_runs, uint64_t total_rows, uint64_t row_begin,
                                    uint64_t chunk_words);
/* The membership check of the reference's build test (validate_elements, /root/reference/tests/ganon-build/GanonBuild.test.cpp:53-98:
 * hash a sequence, bulk_count, add up the counts of its target's bins, compare with the number of hashes) for a flat IBF on the
 * device: *hits = sum over the n hashes (host memory) of the number of `bins` that contain the hash, *missing = hashes no bin
 * contains, *first_missing = the smallest index of one (~0 when none).  `ganon-classify --verify-filter` calls it per target. */
int gn_filter_probe(gn_filter* f, const uint64_t* hashes, uint64_t n, const uint32_t* bins, uint32_t n_bins, uint64_t* hits,
                    uint64_t* missing, uint64_t* first_missing);

/* `ganon-build --hibf` (no counterpart in the reference's own sources: `ganon build --filter-type hibf` runs `raptor prepare / layout /
 * build`, /root/reference/src/ganon/build_update.py:411-518; the index it leaves is what GanonClassify.cpp:875-938 reads).
 * gn_hashes_union: the ascending union of n_sets ASCENDING hash sets in host memory (sets[i][0 .. sizes[i])) and its size -- the exact
 * cardinality of a merged bin.  out may be NULL for the size alone (GN_EOVERFLOW with *n_union set when cap is too small).  At most
 * 2^31 - 1 hashes over all sets of one call (GN_ERANGE beyond).
 * gn_filter_emplace_path: inserts n_sets hash sets -- set s = hashes[set_off[s] .. set_off[s + 1]), ascending -- into an HIBF created
 * with rows == NULL, each along its whole root-to-leaf path in one launch: paths[s * depth + d] says where set s goes in one IBF of
 * the tree -- hash i of the set into bin first_bin + i / hashes_per_bin (a user bin's run of n_bins bins in its leaf IBF, the rule
 * of gn_filter_emplace_split), or, with n_bins == 1, every hash into first_bin (a single bin; a merged bin above the user bin:
 * inserting every member sets the bits their union would).  n_bins == 0 ends a path shorter than `depth`.  Order of the entries
 * is free; every bin is checked against its IBF before anything is launched. */
typedef struct
{
    uint32_t ibf;            /* index of the IBF in the filter */
    uint32_t first_bin;
    uint32_t n_bins;         /* 0: unused entry */
    uint32_t reserved;
    uint64_t hashes_per_bin; /* ignored when n_bins == 1 */
} gn_path_entry;
int gn_hashes_union(int device, const uint64_t* const* sets, const uint64_t* sizes, uint32_t n_sets, uint64_t* out, uint64_t cap,
                    uint64_t* n_union);
int gn_filter_emplace_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                           uint32_t depth);
/* A tree built in parts (`ganon-build --hibf --hibf-memory / --hibf-devices`; no counterpart in the reference).
 * gn_filter_create_hibf_storage: a zero-filled, STORAGE-ONLY HIBF of n_ibf IBFs without tables (ibfs[i].rows == NULL): hashes can be
 * inserted and rows read back (gn_filter_download_rows, gn_filter_info), no stream can be created on it.  Rows are padded on the
 * device as gn_filter_upload_hibf pads them (gn_hibf_row_stride_words).  Its IBFs need not hang together: a part of a tree is any set
 * of its IBFs, or a range of rows of one.
 * gn_filter_emplace_path_window: gn_filter_emplace_path for such a filter.  Set s is sets[s][0 .. set_sizes[s]), ascending, in host
 * memory, taken by pointer; paths as above, their `ibf` numbering f's IBFs.  IBF j of f stands for rows [row_begin[j], row_begin[j] +
 * its rows) of an IBF of total_rows[j] rows (1 .. 2^32 - 1; both arrays have one entry per IBF of f).  For each hash function the
 * row is that of the WHOLE IBF -- hash_and_fit with total_rows[j] and countl_zero(total_rows[j]) -- and the bit is set at row -
 * row_begin[j] only when the row lies in the piece; nothing else is touched.  With row_begin all 0 and total_rows equal to f's rows
 * the call sets exactly the bits gn_filter_emplace_path sets.  All sets of a call go through two page-locked staging chunks of
 * chunk_hashes hashes (0: 1 Mi), the upload of one under the kernel of the one before, one launch per chunk.  Everything is checked
 * before anything is launched and a refused call writes nothing: GN_EINVAL for a null argument, a filter that is not an HIBF, an
 * IBF or a bin out of range, hashes that do not fit their run, row_begin + rows > total_rows; GN_ERANGE for total_rows >= 2^32. */
int gn_filter_create_hibf_storage(int device, uint32_t n_ibf, const gn_ibf_desc* ibfs, gn_filter** out);
int gn_filter_emplace_path_window(gn_filter* f, const uint64_t* const* sets, const uint64_t* set_sizes, uint32_t n_sets, const gn_path_entry* paths,
                                  uint32_t depth, const uint64_t* total_rows, const uint64_t* row_begin, uint64_t chunk_hashes);
/* The hierarchical build from packed sets (`ganon-build --hibf --hibf-hash-sets packed|spilled`; no counterpart in the reference).  All
 * three take runs as gn_filter_emplace_packed_window takes them: run r is blocks[r][0 .. n_blocks[r]) with word_at counting from
 * payload[r][0], its hashes are those of its blocks behind each other, and a short block may lie in the middle (a target's files' sets).
 * A block with cnt of 0 or over 512, width over 64, or payload words without a payload is GN_EINVAL in each of them.  Only packed bytes
 * cross the link: blocks and payload words go up, a kernel decodes a block per wave.
 * gn_packed_union: the ascending union of all hashes of all runs, packed as ONE set -- word for word what gn_packed_encode makes of
 * gn_hashes_union over the decoded runs (a set is cut every 512 hashes; word_at counts from out_payload[0]).  The runs need not be
 * ascending across blocks (a sort follows): a target of several files goes in as the one run it is.  With out_blocks and out_payload
 * NULL the call answers *n_union, *n_out_blocks and *n_out_words alone (the cardinality of a merged bin).  A result of n hashes has at
 * most ceil(n / 512) blocks and n - ceil(n / 512) words, and n is at most the runs' hashes: buffers can be sized without a first call.
 * GN_EOVERFLOW, with the three sizes set and nothing written, when a buffer is too small; GN_ERANGE beyond 2^31 - 1 hashes in one call, as
 * gn_hashes_union.
 * gn_sketches_create_packed: the handle gn_sketches_create returns, every register equal to that of gn_sketches_create on the decoded
 * runs (sketch r of run r; a run without a block is all zeros).
 * gn_filter_emplace_path_packed_window: gn_filter_emplace_path_window for packed sets -- the same filter kinds, paths, total_rows /
 * row_begin, checks and bits; a set's size is the sum of its blocks' cnt, and hash i of the set is hash i of the run.  With row_begin all 0
 * and total_rows equal to f's rows it sets exactly the bits gn_filter_emplace_path sets.  The two staging chunks hold chunk_words payload
 * words (0: 1 Mi words; at least the 511 words a block can have) and the tables of their blocks.  Everything is checked before anything
 * is launched and a refused call writes nothing. */
int gn_packed_union(int device, const gn_packed_block* const* blocks, const uint64_t* n_blocks, const uint64_t* const* payload, uint32_t n_runs,
                    gn_packed_block* out_blocks, uint64_t cap_blocks, uint64_t* out_payload, uint64_t cap_words, uint64_t* n_union,
                    uint64_t* n_out_blocks, uint64_t* n_out_words);
int gn_filter_emplace_path_packed_window(gn_filter* f, const gn_packed_block* const* blocks, const uint64_t* n_blocks, const uint64_t* const* payload,
                                         uint32_t n_sets, const gn_path_entry* paths, uint32_t depth, const uint64_t* total_rows,
                                         const uint64_t* row_begin, uint64_t chunk_words);

/* `ganon-build --hibf --verify-index`: the insert read back.  Same sets, same paths, same hashes; loads where gn_filter_emplace_path ORs.
 * set s = hashes[set_off[s] .. set_off[s+1]) (host memory; any order, repeats allowed).  A hash is CONTAINED in an entry when, for at
 * least one bin of first_bin .. first_bin + n_bins - 1, all h rows have that bin's bit set (hashes_per_bin is ignored: a foreign
 * builder may have dealt the hashes to the run's bins in another order).  n_bins == 0 ends a path shorter than `depth`, as above; the
 * entries from there on are unused.
 * gn_filter_probe_path:
 *   lost_at[s * depth + d] = hashes of set s not contained in entry d, each entry counted on its own (0 for unused entries); may be NULL
 *   found[s]               = hashes of set s contained in every used entry
 *   first_lost[s]          = smallest index within set s of a hash that is not, ~0 when none
 * gn_filter_probe_paths_shared: the same n probes against each of n_paths paths, found[p] = probes contained in every used entry of
 *   path p.  Results do not depend on the order of the paths; sorted by (leaf ibf, first bin) neighbouring paths share what they read.
 * Both: GN_EINVAL for a filter that is not an HIBF, a null argument (lost_at excepted), an IBF or a bin out of range -- everything is
 * checked before anything is launched.  n_sets == 0, n_paths == 0, n == 0 and empty sets are legal (found 0, first_lost ~0).
 *
 * The probes `ganon-build --verify-index` measures false positives with -- values no (k,w)-minimiser hash with k <= 31 can take,
 * since such a hash is below 4^k <= 2^62: for i = 0 .. P - 1, in 64-bit wrapping arithmetic,
 *     z = (i + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *     probe_i = z | 2^63 */
int gn_filter_probe_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                         uint32_t depth, uint64_t* found, uint64_t* lost_at, uint64_t* first_lost);
int gn_filter_probe_paths_shared(gn_filter* f, const uint64_t* probes, uint64_t n, const gn_path_entry* paths, uint32_t n_paths,
                                 uint32_t depth, uint64_t* found);

/* `ganon-build --hibf --verify-index --verify-memory / --verify-devices`: the two probes on a storage filter whose IBFs are pieces of
 * rows of the tree's IBFs (gn_filter_create_hibf_storage, rows written with gn_filter_write_rows at row - row_begin).  total_rows and
 * row_begin mean what they mean in gn_filter_emplace_path_window; the rows of a hash are those of the WHOLE IBF and a row outside
 * the piece counts as "all bits set".  The answers are carried in host bitmaps the caller owns, all in/out and only ever ANDed into:
 * bit q % 64 of word q / 64 stands for hash (probe) q.  An entry with planes == NULL is taken as a whole piece: a hash that is not
 * contained in it is cleared from `alive`.  An entry with planes is a slab of a cut IBF: plane b (n_bins planes of the bitmap's
 * length, behind each other) keeps "every row of the hash seen so far has the bit of bin first_bin + b"; the caller closes the entry
 * when the IBF's last slab is through -- hit = OR of the planes, alive &= hit (host/hibf_verify_parts.hpp).  Planes start as all ones.
 * gn_filter_probe_path_window: set s = sets[s][0 .. set_sizes[s]) by pointer, as for the windowed insert.
 *   alive[s]               ceil(set_sizes[s] / 64) words; the caller starts it with one bit per hash and the padding bits zero
 *   planes                 NULL, or n_sets * depth pointers: planes[s * depth + d] NULL or n_bins * ceil(set_sizes[s] / 64) words
 *   lost_at[s * depth + d] ADDED to: the hashes of set s not contained in entry d, for entries without planes only
 *   chunk_hashes           hashes of a staging chunk (0: 1 Mi), rounded up to a multiple of 512: every wave's 512 hashes start at a
 *                          multiple of 512 of their set and own whole words of its bitmaps
 * gn_filter_probe_paths_shared_window: the same n probes against each of n_paths paths.
 *   alive                  n_paths * ceil(n / 64) words, path p's bitmap at p * ceil(n / 64)
 *   planes                 NULL, or n_paths * depth pointers: planes[p * depth + d] NULL or n_bins * ceil(n / 64) words
 *   A probe that is cleared from `alive` already is not looked at again, so the planes of a path say nothing about it.
 * Both check everything before anything is launched and a refused call changes no buffer: GN_EINVAL for a null argument (planes
 * excepted), a filter that is not an HIBF, an IBF or a bin out of range, row_begin + rows > total_rows, IBFs of unequal hash
 * functions; GN_ERANGE for total_rows >= 2^32.  n_sets == 0, n_paths == 0, n == 0 and empty sets are legal and change nothing. */
int gn_filter_probe_path_window(gn_filter* f, const uint64_t* const* sets, const uint64_t* set_sizes, uint32_t n_sets, const gn_path_entry* paths,
                                uint32_t depth, const uint64_t* total_rows, const uint64_t* row_begin, uint64_t* const* alive,
                                uint64_t* const* planes, uint64_t* lost_at, uint64_t chunk_hashes);
int gn_filter_probe_paths_shared_window(gn_filter* f, const uint64_t* probes, uint64_t n, const gn_path_entry* paths, uint32_t n_paths,
                                        uint32_t depth, const uint64_t* total_rows, const uint64_t* row_begin, uint64_t* alive,
                                        uint64_t* const* planes);

/* `ganon-build --hibf --update`: what an index on the device says about itself, and its move into a wider one (no counterpart in the
 * reference: `ganon update` rebuilds the filter, update() in src/ganon/build_update.py).
 * gn_filter_bin_popcounts: counts[b], for every b below the bins of IBF `ibf_idx` (host memory, that many entries), = the number of
 *   rows of the IBF whose bit b is set -- how full technical bin b is; a .hibf records nothing else about it.  ibf_idx = 0 of a flat
 *   filter (one created without a bin map included), any IBF of an HIBF.  The device's padded row stride (gn_hibf_row_stride_words)
 *   does not show: padding bins and padding words are not reported.  Every word of the IBF is read once; exact, whatever the order
 *   the device adds in (integers).  GN_EINVAL for a null argument or an IBF the filter does not have.
 * gn_filter_copy_ibf: IBF src_ibf of `src` into IBF dst_ibf of `dst`, device to device: words [0, W_src) of every row are the
 *   source's (W = ceil(bins / 64)), the words from there to the destination's row stride are zero -- bin b of the source is bin b of
 *   the destination, every further bin is empty.  The source's last word is taken as it is: its padding bins are clear in a filter
 *   that was finalised or streamed from a file.  GN_EINVAL unless both are HIBF filters on the same device, the two IBFs have the
 *   same number of rows and of hash functions, and the destination has at least the source's words a row; everything is checked
 *   before anything is launched.  Returns when the copy is complete. */
int gn_filter_bin_popcounts(const gn_filter* f, uint32_t ibf_idx, uint64_t* counts);
int gn_filter_copy_ibf(gn_filter* dst, uint32_t dst_ibf, const gn_filter* src, uint32_t src_ibf);

/* `ganon-build --hibf --update --extend`: more hashes for user bins that are filled already.  gn_filter_emplace_path cannot do it: it
 * deals hash i to bin first_bin + i / hashes_per_bin, a reader sums the counts of a user bin's technical bins, and a hash that lands in a
 * second bin of the run is counted twice.  How the run was dealt is not known either, so what a bin still takes is said by the caller.
 * gn_filter_extend_path: sets and paths as gn_filter_emplace_path takes them -- entry 0 of a path is the user bin's leaf run, the
 *   entries above it are merged bins (n_bins == 1), n_bins == 0 ends a path, hashes_per_bin is ignored -- and every set STRICTLY
 *   ascending.  deal[deal_off[s] + j] is the quota of bin first_bin + j of set s's leaf run; deal_off[s + 1] - deal_off[s] is that
 *   run's n_bins.  All of the following is taken against the filter as it is when the call starts:
 *     a hash of set s is PRESENT when it is contained in entry 0 (the rule of gn_filter_probe_path: for at least one bin of the run all
 *       h rows have that bin's bit set); the ABSENT hashes of the set, in set order, have ranks 0 .. a_s - 1
 *     the absent hash of rank r is ORed into the leaf bin j with cum[j] <= r < cum[j + 1], cum the running sum of the set's quotas
 *     a present hash sets no leaf bit: a reader finds it where it is
 *     every hash of the set, present or not, is ORed into every merged entry above the leaf (a hash that is falsely present in the leaf
 *       may be missing above)
 *   GN_EINVAL, and NOTHING written, when the quotas of a set do not sum to a_s (the message names the set and both numbers), for a
 *   filter that is not an HIBF, a null argument, a set that is not strictly ascending, a quota list that is not as long as the run, a
 *   run of several bins above the leaf, an IBF or a bin out of range: every check and the whole marking sweep come before the first OR.
 *   n_sets == 0 and empty sets are legal.  The result is a function of the arguments and the filter's bits alone. */
int gn_filter_extend_path(gn_filter* f, const uint64_t* hashes, const uint64_t* set_off, uint32_t n_sets, const gn_path_entry* paths,
                          uint32_t depth, const uint64_t* deal_off, const uint64_t* deal);

/* `ganon-build --hibf --update --remove`: the move of an IBF into another one that leaves bins out (no counterpart in the reference).
 * gn_filter_copy_ibf_spans: for every row, bit dst_first + j of IBF dst_ibf of `dst` is bit src_first + j of IBF src_ibf of `src`, for
 *   every j < n_bins of every span; every other bit of the destination's row is zero, up to its padded row stride
 *   (gn_hibf_row_stride_words): the padding bins of the last word and whatever the destination held before included.  The spans are
 *   ascending and disjoint in the destination; their source positions are free (a permutation of runs is legal, and so is one source
 *   bin in several spans).  The destination may have fewer or more bins than the source.  The one span {0, 0, bins of the source}
 *   gives what gn_filter_copy_ibf gives.  n_spans == 0 zeroes the destination (`spans` may then be NULL).
 *   GN_EINVAL, with everything checked before anything is launched (a refused call writes nothing): a null argument; a filter that is
 *   not an HIBF, or two filters on different devices; an IBF out of range, or an IBF onto itself; differing rows or hash functions; a
 *   span of 0 bins; a span beyond the source's or the destination's bins; destination spans that overlap or do not ascend.
 *   Returns when the copy is complete. */
typedef struct
{
    uint32_t src_first, dst_first, n_bins, reserved;
} gn_bin_span;
int gn_filter_copy_ibf_spans(gn_filter* dst, uint32_t dst_ibf, const gn_filter* src, uint32_t src_ibf, const gn_bin_span* spans,
                             uint32_t n_spans);

/* `ganon-build --hibf --update --fold`: the merged bins above groups of bins of an IBF (no counterpart in the reference).
 * gn_filter_fold_ibf: for every row, bit dst_first + g of IBF dst_ibf of `dst` is ORed with the OR of bits src_first .. src_first +
 *   n_bins - 1 of the row of IBF src_ibf of `src`, over all members of group g, for every g < n_groups; no other bit of the destination
 *   changes, and what the destination held stays (the call is an OR).  A hash's row depends on the hash, the seed and the IBF's row count
 *   only, so with equal rows this is, bit for bit, the merged bin a build would have put above the group.  The members ascend and are
 *   disjoint in the source; their groups are free in order, and a group may have several members.  n_groups == 0 does nothing.
 *   GN_EINVAL, with everything checked before anything is launched (a refused call writes nothing): a null argument; a filter that is
 *   not an HIBF, or two filters on different devices; an IBF out of range, or an IBF onto itself; differing rows or hash functions; a
 *   member of 0 bins or beyond the source's bins; members that overlap or do not ascend; a group >= n_groups, or a group without a
 *   member; dst_first + n_groups beyond the destination's bins.  GN_ERANGE for more groups than one call holds (above 170 000).
 *   Returns when the fold is complete. */
typedef struct
{
    uint32_t src_first, n_bins, group, reserved;
} gn_fold_member;
int gn_filter_fold_ibf(gn_filter* dst, uint32_t dst_ibf, uint32_t dst_first, uint32_t n_groups, const gn_filter* src, uint32_t src_ibf,
                       const gn_fold_member* members, uint32_t n_members);

/* `ganon-build --hibf --layout sketch | similarity`: HyperLogLog sketches of hash sets and the estimated cardinality of unions of neighbouring
 * sketches -- what a layout search asks n * width times (raptor gets its tree from chopper's sketches through `raptor layout`,
 * /root/reference/src/ganon/build_update.py:411-518).  The estimates choose the tree only: the IBFs are sized from gn_hashes_union.
 *
 * A sketch is GN_SKETCH_M = 4096 registers of one byte.  For a hash h of the set:
 *     x = h;  x ^= x >> 33;  x *= 0xff51afd7ed558ccd;  x ^= x >> 33;  x *= 0xc4ceb9fe1a85ec53;  x ^= x >> 33;     (64-bit, wrapping:
 *                                                     murmur3's finaliser -- minimiser hashes are not uniform)
 *     index = x >> 52                                 (the top 12 bits)
 *     rest  = x & (2^52 - 1);  rank = 52 when rest == 0, else (leading zeros of rest as a 52-bit number) + 1     (1 .. 52)
 *     register[index] = max(register[index], rank)
 * An empty set is all zeros.  Register r of sketch i is byte i * 4096 + r of what gn_sketches_download returns.
 *   gn_sketches_create       sets[i][0 .. sizes[i]) in host memory (order and repeats inside a set do not matter), one sketch each,
 *                            kept on `device`
 *   gn_sketches_download     registers of sketches first .. first + n - 1 (tests)
 *   gn_sketches_union_table  `order` = n sketch indices (each below the handle's number of sketches; repeats allowed).  For every
 *                            start j in [j0, j1) and every l in [1, min(width, n - j)], out[(j - j0) * width + l - 1] = the largest of
 *                            E(j, 1) .. E(j, l), where E(j, l) estimates the union of sketches order[j .. j + l); entries with
 *                            l > n - j are 0.  So every row is non-decreasing up to its end.  At most GN_SKETCH_TABLE_MAX entries
 *                            ((j1 - j0) * width) in one call, GN_ERANGE beyond: rows are independent, tile over the starts.
 *   gn_sketches_pair_table   (`--layout similarity`) `idx` = m sketch indices (each below the handle's number of sketches, GN_EINVAL
 *                            otherwise; repeats allowed).  out[a * m + b] = E of the union of the two sketches idx[a] and idx[b],
 *                            for every a and b below m: the plain E of the pair -- no running maximum as in the union table.  The
 *                            table is symmetric, and its diagonal is E of the single sketch.  At most GN_SKETCH_TABLE_MAX entries
 *                            (m * m, so m <= 4096) in one call, GN_ERANGE beyond.  m == 0 writes nothing and returns GN_OK.
 * E from the union's registers U[r] = max over the sketches of register r, with m = 4096:
 *     Z = number of r with U[r] == 0;  S = sum over r of 2^(52 - U[r]) as an integer (below 2^64 unless Z == m)
 *     Z == m: E = 0.  Otherwise raw = num / (double)S, both the conversion and the division rounded to nearest, with
 *     num = alpha * 2^76 (= alpha * m^2 * 2^52), alpha = 0.7213 / (1.0 + 1.079 / 4096.0) in double arithmetic;
 *     value = raw <= 10240.0 (2.5 m) and Z > 0 ? 4096.0 * log(4096.0 / (double)Z) : raw
 *     E = value rounded to the nearest integer, ties to even, as uint64
 * (the logarithms come from a table of 4097 doubles the host computes with the C library's log(); the device calls none). */
#define GN_SKETCH_M 4096u
#define GN_SKETCH_TABLE_MAX (1ull << 24)
typedef struct gn_sketches gn_sketches;
int gn_sketches_create(int device, const uint64_t* const* sets, const uint64_t* sizes, uint32_t n_sets, gn_sketches** out);
/* (from packed runs: see gn_packed_union above) */
int gn_sketches_create_packed(int device, const gn_packed_block* const* blocks, const uint64_t* n_blocks, const uint64_t* const* payload, uint32_t n_runs,
                              gn_sketches** out);
int gn_sketches_free(gn_sketches* s);
int gn_sketches_download(gn_sketches* s, uint32_t first, uint32_t n, uint8_t* out);
int gn_sketches_union_table(gn_sketches* s, const uint32_t* order, uint32_t n, uint32_t j0, uint32_t j1, uint32_t width, uint64_t* out);
int gn_sketches_pair_table(gn_sketches* s, const uint32_t* idx, uint32_t m, uint64_t* out);

/* Parity / debugging taps (tests only): minimiser hashes of the resident batch in emission order
 * (hash_off[n_reads+1]; hashes[cap]) and dense per-bin counts of reads [read_begin, read_end)
 * (flat IBF: uint16[bins] per read == counting_agent::bulk_count; HIBF: uint16[n_user_bins] per read
 * == counting_agent_type::bulk_count(values, T)). */
int gn_stream_fetch_hashes(gn_stream* s, uint64_t* hash_off, uint64_t* hashes, uint64_t cap, uint64_t* n_total);
int gn_stream_dense_counts(gn_stream* s, uint32_t read_begin, uint32_t read_end, uint16_t* counts);

int gn_stream_timings(gn_stream* s, gn_timings* t);
/* Flat IBF: units (read x column slice) of the last batch that the fast count kernel's screen-only launch left to the launch that
 * follows it -- reads without a screen in the launch's table, aborted screens.  0 where that kernel does not run. */
int gn_stream_screen_deferred(gn_stream* s, uint64_t* units);
/* Flat IBF, four hash functions: from `bytes` of row storage on, a filter's fast count launches take the stream kernels -- the same
 * kernels with non-temporal row loads, for a filter far past the caches, whose lines are read once (csrc/gn_row_policy.h).  Default:
 * 2 GiB, or $GANON_HIP_STREAM_ROWS_MIN_BYTES as it was when the library was loaded; 0 = every launch that has a stream instance.
 * Results and the bytes requested do not depend on it.  Call it while no launch on the filter is in flight. */
int gn_filter_set_stream_rows_min_bytes(gn_filter* f, uint64_t bytes);
/* *streamed = 1 when the fast count launches of the last classify took the stream kernels, else 0 (plain row loads: a small filter,
 * an HIBF, a shape without a stream instance, the switch stream_rows). */
int gn_stream_rows_streamed(gn_stream* s, int* streamed);
/* HIBF only: the last batch per tree level (level 0 = the top IBF) -- duration of the level's kernels, algorithmic row
 * bytes of the level (they add up to gn_timings.algo_bytes), bytes of the IBFs at that depth and their usual row width.
 * A level whose tables fit the 256 MiB Infinity Cache is not bound by HBM; the roofline is stated per level for that
 * reason.  Arrays of `cap` entries; *n_levels = levels of the filter's tree (at most 8 are timed separately). */
int gn_stream_hibf_levels(gn_stream* s, uint32_t* n_levels, float* ms, uint64_t* algo_bytes, uint64_t* table_bytes,
                          uint32_t* row_bytes, uint32_t cap);

/* ... and the same row requests in the 128-byte lines the rows occupy (a 32-byte row moves a line, a 136-byte row two): with IBFs of
 * different widths on one level this, not row_bytes, is what the level's physical rate is computed from. */
int gn_stream_hibf_level_lines(gn_stream* s, uint64_t* line_bytes, uint32_t cap);

/* ---- gzip input inflated on the device (csrc/gn_inflate.hip) ------------------------------------------------------------------
 * Replaces, for `reads.fq.gz` / `reads.fa.gz`, the zlib stream the reference reads its input through
 * (seqan3::sequence_file_input over a gz stream in parse_reads, /root/reference/src/ganon-classify/GanonClassify.cpp:1220-1287;
 * its one decompression thread, :1433): the caller feeds the file's bytes as they are, the device finds deflate block starts,
 * decodes the chunks between them in parallel and returns the text -- the same bytes zlib's inflate() yields for the file
 * (every member; what follows the last member is ignored like gzip does).  Every member's CRC-32 and ISIZE are checked.
 *   gn_inflate_create   compressed_bytes = size of the file; chunk_bytes = compressed bytes per parallel chunk (0: 32 KiB);
 *                       step_bytes = compressed bytes decoded per gn_inflate_step (0: 128 MiB for files below 1.5 GB, 256 MiB above; at most 8192 chunks).  The whole compressed file
 *                       stays resident in HBM (files of 64 GiB and more: GN_ERANGE).
 *   gn_inflate_feed     appends the next n bytes of the file (host memory; returns when `data` may be reused)
 *   gn_inflate_step     decodes the next step: every chunk whose bytes, and 4 MiB behind them, are fed -- all of the rest once the
 *                       whole file is.  *n_text = bytes of text this step produced (they follow the previous step's), *done = 1
 *                       after the last member's trailer.  Blocks until the text is complete in device memory.
 *   gn_inflate_text     copies [off, off + n) of the LAST step's text to host memory
 *   gn_inflate_text_device   the last step's text in device memory (valid until the step after the next one begins)
 * GN_ERANGE from gn_inflate_step: damaged / truncated data, a wrong CRC-32 or ISIZE, or data this decoder is not made for (more than
 * 8-fold expansion, hardly any dynamic-Huffman blocks): the caller reads the file with its host inflater instead -- nothing
 * that was returned before is wrong, and nothing is returned that was not decoded. */
typedef struct gn_inflate gn_inflate;
typedef struct gn_inflate_stats
{
    uint64_t steps, chunks, fixups, markers, members, text_bytes;
    double   ms_decode, ms_chain, ms_resolve, ms_step_wall;
    /* a library built with -DGI_PROF=1 (scripts/inflate_variants.sh; zeros otherwise), summed over the chunks (wave-milliseconds): block search screen, headers of search candidates, block headers, Huffman decoding,
     * placing the tokens (LZ77 copies), flushes, whole chunk; [7] unused */
    double   prof_ms[8];
} gn_inflate_stats;
int gn_inflate_create(int device, uint64_t compressed_bytes, uint32_t chunk_bytes, uint64_t step_bytes, gn_inflate** out);
int gn_inflate_destroy(gn_inflate* z);
int gn_inflate_feed(gn_inflate* z, const uint8_t* data, uint64_t n);
int gn_inflate_step(gn_inflate* z, uint64_t* n_text, int* done);
int gn_inflate_text(gn_inflate* z, uint8_t* dst, uint64_t off, uint64_t n);
int gn_inflate_text_device(gn_inflate* z, const uint8_t** text, uint64_t* n);
int gn_inflate_get_stats(gn_inflate* z, gn_inflate_stats* out);
/* Batches for the classifier straight from the device: where do records begin in the last step's text?
 *   gn_inflate_cuts       cuts[0 .. *n_cuts): ascending offsets into the last step's text, each the first byte behind a newline whose
 *                         number (from 1, counted from the text's first byte) is a multiple of lines_per_record (4: FASTQ, 2: two-line
 *                         FASTA) -- the first such offset at or behind every multiple of piece_bytes, and the last one of the text.
 *                         The text's first byte must begin a record (true for a file's first step; later: gn_inflate_set_carry).
 *   gn_inflate_set_carry  the last n_tail bytes of the last step's text (the record the step's end cuts) are what the NEXT step's text
 *                         begins with: its n_text counts them, its text holds them in front. */
int gn_inflate_cuts(gn_inflate* z, uint32_t lines_per_record, uint64_t piece_bytes, uint64_t* cuts, uint32_t cap, uint32_t* n_cuts);
/* ... for the two files of paired reads (parse_reads takes file 2 with take(n_reads), GanonClassify.cpp:1240-1252: pairs go by record
 * NUMBER): gn_inflate_cuts_lines also says how many lines lie in front of every cut (cut_lines[i], counted from the text's first byte);
 * gn_inflate_cut_at_lines answers, for the mate file's text, where those many lines end: offsets[i] = first byte behind line number
 * lines[i] (0 for 0 lines, ~0 when the text holds fewer), *total_lines = newlines in the text. */
int gn_inflate_cuts_lines(gn_inflate* z, uint32_t lines_per_record, uint64_t piece_bytes, uint64_t* cuts, uint64_t* cut_lines, uint32_t cap, uint32_t* n_cuts);
int gn_inflate_cut_at_lines(gn_inflate* z, const uint64_t* lines, uint32_t n_lines, uint64_t* offsets, uint64_t* total_lines);
int gn_inflate_set_carry(gn_inflate* z, uint64_t n_tail);
/* One file, several devices.  A step's decode depends on nothing before it; the pieces that put a step's text together need four things
 * of the step before: the stream's bit position, the open member's length and CRC-32 so far, the 32 KiB window, and the text the step's
 * end cut off.  So N inflaters created for the SAME file (same sizes), each fed the whole file, can take its steps in turn:
 *   gn_inflate_set_turns(z_i, N, i)   before the first step: z_i will run steps i, i + N, ... (sizes its decodes-ahead by that; only
 *                                      turn 0's first step is the file's short first step)
 *   gn_inflate_handoff(from, to)      after gn_inflate_step(from) [+ gn_inflate_cuts / gn_inflate_set_carry(from)], before
 *                                      gn_inflate_step(to): copies those four things device to device (32 KiB + the carried record)
 * The text of step k then lies on device k mod N -- where the worker of that device classifies it without a peer copy.  With one
 * inflater the file is bound by that device's decode rate (31-37 GB/s of text); with N by the serial passes (order, windows, resolve,
 * CRC: ~7 ms per 0.9 GB of text).  The reference reads a .gz through one zlib stream (GanonClassify.cpp:1220-1287,1433). */
int gn_inflate_set_turns(gn_inflate* z, uint32_t n_turns, uint32_t my_turn);
int gn_inflate_handoff(gn_inflate* from, gn_inflate* to);

#ifdef __cplusplus
}
#endif
#endif
