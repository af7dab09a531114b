/* hbam.h — C ABI of the MI355X-native BAM read path (libhbam.so).
 *
 * Drop-in boundary for Hadoop-BAM's BAM input path.  The reference's Java classes
 * (org.seqdoop.hadoop_bam.*) keep their API and bind these entry points through
 * Panama FFI / JNI.  Every entry point names the reference
 * interface it replaces.  Plain C: pointers + sizes, no C++ or torch types, no
 * exceptions across the boundary.  Negative return codes map 1:1 onto the Java
 * exception the reference raises at the same point:
 *
 *   HBAM_EIO          java.io.IOException
 *   HBAM_ETRUNC       htsjdk.samtools.FileTruncatedException
 *   HBAM_EFORMAT      htsjdk.samtools.SAMFormatException
 *   HBAM_ERUNTIMEIO   htsjdk.samtools.util.RuntimeIOException
 *   HBAM_EEOF         htsjdk.samtools.util.RuntimeEOFException
 *   HBAM_EREFID       IllegalArgumentException (reference index not in dictionary)
 *   HBAM_EDATA        RuntimeException(java.util.zip.DataFormatException)
 *   HBAM_EINDEX       IndexOutOfBoundsException
 *   HBAM_ETRIBBLE     htsjdk TribbleException (BCF, text VCF)
 *   HBAM_ERUNTIME     another RuntimeException out of BCF2Codec.decode (BCF, unpinned); the
 *                     NullPointerException after VCFCodec.decode returns null (text VCF)
 *   HBAM_ENULL        NullPointerException (multi-input Sort's group rewrite, cli/Utils.java:316-323)
 *   HBAM_ECLASSCAST   ClassCastException (an RG / PG attribute that is not a string)
 *   HBAM_ESEQFORMAT   org.seqdoop.hadoop_bam.FormatException (FASTQ, QSEQ)
 *   HBAM_ENUMBER      NumberFormatException (Integer.parseInt in the FASTQ / QSEQ readers)
 *
 * Library-specific codes (no reference counterpart): HBAM_ENOMEM, HBAM_EUNSUPPORTED
 * (BGZF block with ISIZE > 65536; SAM text the encoder does not restate; the FASTQ / QSEQ inputs
 * listed at hbam_fastq_decode_split), HBAM_EDEVICE (HIP
 * error), HBAM_EINVAL, HBAM_EMORE
 * (the compressed window handed in ends before the split's last record).
 *
 * Inputs: an argument with `on_device` = 0 is host memory, copied in by the call; with
 * `on_device` = 1 it is a device pointer read in place, and the kernels read whole 16-byte
 * quads and fixed-size windows past the last byte, so 64 readable bytes must follow `len`
 * (their contents do not matter).  Host inputs get that padding from the library.
 *
 * Threading: a context owns one HIP stream and is single-threaded; separate contexts
 * (one per Hadoop task thread) are independent.  Device buffers returned in
 * hbam_columns are owned by the context and stay valid until the next decode call on
 * that context or hbam_release_columns().
 */
#ifndef HBAM_H
#define HBAM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBAM_OK 0
#define HBAM_EIO (-1)
#define HBAM_ETRUNC (-2)
#define HBAM_EFORMAT (-3)
#define HBAM_ERUNTIMEIO (-4)
#define HBAM_EEOF (-5)
#define HBAM_EREFID (-6)
#define HBAM_EDATA (-7)
#define HBAM_ENOMEM (-8)
#define HBAM_EUNSUPPORTED (-9)
#define HBAM_EDEVICE (-10)
#define HBAM_EINVAL (-11)
#define HBAM_EMORE (-12)
#define HBAM_EINDEX (-13) /* IndexOutOfBoundsException (Summarize.java:715 on a record without a range) */
#define HBAM_ETRIBBLE (-14) /* htsjdk TribbleException (BCF2Codec: unreadable / inconsistent BCF record) */
#define HBAM_ERUNTIME (-15) /* another RuntimeException escaping BCF2Codec.decode (restated, unpinned) */
#define HBAM_ENULL (-16) /* NullPointerException (cli/Utils.java:316-323: a group lookup without a table) */
#define HBAM_ECLASSCAST (-17) /* ClassCastException ((String) of a non-string RG / PG attribute) */
#define HBAM_ESEQFORMAT (-18) /* FormatException (FormatException.java): QSEQ field count, base quality range */
#define HBAM_ENUMBER (-19) /* NumberFormatException out of Integer.parseInt (FASTQ Illumina id, QSEQ ints) */

typedef struct hbam_ctx hbam_ctx;

/* Configuration knobs (Hadoop Configuration properties in the Java shim):
 *   check_crc      hadoopbam.hip.check-crc: BlockCompressedInputStream.setCheckCrcs
 *                  (off in BAMRecordReader, on in the split guessers)
 *   validate_refs  1 = BAMRecordCodec(header) as BAMRecordReader.java:130 builds it
 *                  (refID / mate refID must lie in [-1, n_ref)); 0 = LazyBAMRecordFactory */
typedef struct hbam_opts {
  int32_t check_crc;
  int32_t validate_refs;
  int32_t reserved[14];  /* must be zero */
} hbam_opts;

typedef struct hbam_header {
  int32_t l_text;
  int32_t n_ref;           /* SAMFileHeader.getSequenceDictionary().size() */
  uint64_t header_ulen;    /* uncompressed bytes of the BAM header */
  uint64_t first_voffset;  /* virtual offset of the first record */
} hbam_header;

typedef struct hbam_block {
  uint64_t coff;   /* file offset of the BGZF block */
  uint32_t clen;   /* BSIZE + 1 */
  uint32_t isize;  /* ISIZE footer */
  uint32_t crc;    /* CRC32 footer */
  uint32_t pad;
} hbam_block;

/* Decoded split, struct-of-arrays.  In hbam_decode_split's output every pointer is a
 * device pointer owned by the context; after hbam_columns_to_host they are host
 * pointers owned by the caller (free with hbam_free_host_columns).  In the host copy, ubuf
 * holds exactly the records' bytes (each record's block_size field + record, i.e. the
 * SAMRecordWritable wire form) and rec_off is relative to it. */
typedef struct hbam_columns {
  uint64_t n_records;
  int32_t status;       /* HBAM_OK, or the exception nextKeyValue()/initialize() raises */
  int32_t pad0;
  uint64_t err_record;  /* record index at which `status` is raised */
  uint64_t* voffset;    /* bci.getFilePointer() before each record */
  int64_t* key;         /* BAMRecordReader.getKey(record) (LongWritable key) */
  uint64_t* rec_off;    /* offset of each record's block_size field in ubuf */
  uint8_t* ubuf;        /* inflated stream of the split (SAMRecordWritable payloads) */
  uint64_t ubuf_len;
  int32_t* block_size;
  int32_t* ref_id;
  int32_t* pos;         /* 0-based */
  uint8_t* l_read_name;
  uint8_t* mapq;
  uint16_t* bin;
  uint16_t* n_cigar;
  uint16_t* flag;
  int32_t* l_seq;
  int32_t* next_ref_id;
  int32_t* next_pos;
  int32_t* tlen;
  uint8_t* layout_ok;   /* 0: variable block inconsistent with the fixed lengths */
  uint64_t* name_off;   /* n+1 offsets into names (l_read_name bytes each, incl. NUL) */
  uint8_t* names;
  uint64_t* cigar_off;  /* n+1 offsets (in u32 ops) into cigars */
  uint32_t* cigars;
  uint64_t* seq_off;    /* n+1 offsets into seq (unpacked "=ACMGRSVTWYHKDBN") and qual */
  uint8_t* seq;
  uint8_t* qual;
  uint64_t* aux_off;    /* n+1 offsets into aux (raw typed tags) */
  uint8_t* aux;
} hbam_columns;

/* Per-stage device times of the last call, milliseconds (HIP events on the context's
 * stream), for the roofline report. */
typedef struct hbam_timing {
  double scan_ms, inflate_ms, crc_ms, walk_ms, decode_ms, pools_ms, total_ms;
  double huffman_ms, resolve_ms; /* inflate = Huffman pass (k_inflate_tokens) + k_resolve (LZ77) */
  uint64_t n_blocks, comp_bytes, ubuf_bytes, n_records, pool_bytes;
  double exchange_ms; /* hbam_sort_exchange: the grouped ncclSend/ncclRecv on the context stream */
} hbam_timing;

/* ---- context ---------------------------------------------------------------------- */
hbam_ctx* hbam_create(int device_ordinal, const hbam_opts* opts);
void hbam_destroy(hbam_ctx* ctx);
const char* hbam_last_error(const hbam_ctx* ctx);
void* hbam_stream(hbam_ctx* ctx); /* hipStream_t of the context */
int hbam_get_timing(const hbam_ctx* ctx, hbam_timing* out);

/* ---- device staging (the Java shim maps HDFS bytes into pinned buffers) ---------- */
int hbam_upload(hbam_ctx* ctx, const uint8_t* host, uint64_t len, uint8_t** dev_out);
int hbam_device_free(hbam_ctx* ctx, uint8_t* dev);
/* page-lock / release a caller-owned host range (hipHostRegister) so hbam_split_next's window
 * copies run asynchronously beside the decode; memory pinned by another HIP runtime in the
 * process (PyTorch-ROCm's) is pageable to this library */
int hbam_host_register(hbam_ctx* ctx, void* host, uint64_t len);
int hbam_host_unregister(hbam_ctx* ctx, void* host);
/* copy `bytes` of library-owned device memory (e.g. an f-4 output) to host memory, ordered after
 * the context's work */
int hbam_download(hbam_ctx* ctx, const void* dev, uint64_t bytes, void* host);

/* ---- SAMHeaderReader.readSAMHeaderFrom (util/SAMHeaderReader.java:53-72) ----------
 * `file` holds the start of the BAM file (host or device per `on_device`). */
int hbam_parse_header(hbam_ctx* ctx, const uint8_t* file, int on_device, uint64_t len,
                      hbam_header* out);

/* ---- BGZF block table: [htsjdk] BlockCompressedInputStream.readBlock framing;
 * util/BGZFBlockIndexer.java:130-181 (skipBlock).  Chain from offset 0 of `comp`. */
int hbam_scan_blocks(hbam_ctx* ctx, const uint8_t* comp, int on_device, uint64_t len,
                     uint64_t base_off, hbam_block* out, uint64_t cap, uint64_t* n_out);

/* The block table every decode builds first: the chain from offset `start` of the window
 * comp[0, len), block offsets relative to `comp`, at most `cap` of them copied to `out` (may be
 * NULL).  end_pos is where the chain stops and end_code what reading a block there raises
 * (HBAM_EEOF: clean end of file; HBAM_EMORE: the window ends mid-chain and is not the file's
 * end).  Windows of 256 MiB and more are built by the sparse form (one 64 KiB scan window and
 * one chain walker per segment; env HBAM_CHAIN_SEG = segment bytes, which also admits every
 * size; HBAM_CHAIN_MIN = smallest window in bytes); whatever it does not accept, smaller windows,
 * and everything under env HBAM_CHAIN_DENSE=1 goes through the dense scan of every byte
 * position.  The three are read when the context is created.  sparse = 1 when the sparse form
 * answered this call; fallback_flags = why it did not (bit 0 a scan window without a candidate,
 * 1 with more than 4, 2 every candidate of a segment derailed, 3 hop cap, 4 stitch mismatch; 0
 * when it was not tried).  sparse_calls / dense_calls count the context's chain builds so
 * far, by all entry points.  comp = NULL: the counters and the last build's flags only. */
typedef struct hbam_chain_info {
  uint64_t n_blocks, end_pos;
  int32_t end_code, sparse;
  uint32_t fallback_flags, pad;
  uint64_t sparse_calls, dense_calls;
} hbam_chain_info;
int hbam_chain_table(hbam_ctx* ctx, const uint8_t* comp, int on_device, uint64_t len, uint64_t start,
                     int window_is_file_end, hbam_block* out, uint64_t cap, hbam_chain_info* info);

/* ---- batched inflate: [htsjdk] BlockGunzipper.unzipBlock (JDK zlib).  Blocks are
 * relative to `comp`; output concatenated into host `out` at out_off (n+1 entries,
 * exclusive scan of ISIZE, filled by the call).  blk_status: 0, HBAM_EFORMAT (short
 * output / CRC mismatch), HBAM_EDATA (DataFormatException). */
int hbam_inflate(hbam_ctx* ctx, const uint8_t* comp, int on_device, uint64_t comp_len,
                 const hbam_block* blks, uint64_t n, int check_crc, uint8_t* out,
                 uint64_t out_cap, uint64_t* out_off, int32_t* blk_status);

/* ---- BAMRecordReader.initialize + nextKeyValue loop (BAMRecordReader.java:108-188)
 * over FileVirtualSplit [v_start, v_end) (FileVirtualSplit.java:38-92).
 * `comp` = bytes [comp_base, comp_base+comp_len) of a file of length file_len (a window).
 * n_ref < 0: parse it from the header (comp must then start at file offset 0).
 * Windows: when the window ends before the split does, out->status = HBAM_EMORE, the first
 * n_records records are final, and voffset[n_records] (device) is the virtual offset to
 * resume from (v_start when n_records == 0 and no column was produced: the window is too
 * small); the next window must start at or before that offset's BGZF block.  Resuming at
 * that offset gives exactly the records (and the exception) one whole-file call gives. */
int hbam_decode_split(hbam_ctx* ctx, const uint8_t* comp, int on_device, uint64_t comp_base,
                      uint64_t comp_len, uint64_t file_len, uint64_t v_start, uint64_t v_end,
                      int32_t n_ref, hbam_columns* out);
int hbam_columns_to_host(hbam_ctx* ctx, const hbam_columns* dev, hbam_columns* host);
/* Records-only host copy for the drop-in reader: BAMRecordReader.nextKeyValue
 * (BAMRecordReader.java:172-188) hands out one record at a time and needs only its bytes, its key
 * and (getProgress, :157-168) its virtual offset.  host gets n_records, status, err_record, key,
 * voffset, block_size, rec_off (relative to host->ubuf) and ubuf = exactly the records' bytes
 * (each record's block_size field + record); every other pointer is NULL.  The arrays live in
 * pinned host memory owned by the context, valid until the next hbam_records_to_host or
 * hbam_destroy on it (never pass them to hbam_free_host_columns): one consumer per context — a
 * reader among several on one context takes hbam_split_records_to_host instead.  Copies 28 B per
 * record plus the record bytes (columns_to_host copies every pool too: about twice as much).
 * Precondition: `dev` holds a decoded split's columns (hbam_decode_split, hbam_split_next,
 * hbam_rewrite_groups), whose records lie back to back in ubuf in index order; columns whose
 * records are permuted or not contiguous return HBAM_EINVAL. */
int hbam_records_to_host(hbam_ctx* ctx, const hbam_columns* dev, hbam_columns* host);
/* Streamed split read: BAMRecordReader over FileVirtualSplit
 * [v_start, v_end) of a file the caller holds in host memory (e.g. mmap; only the split's
 * windows are copied, see hbam_split_open_reader for the bound), decoded in windows
 * of about window_bytes compressed bytes.  While window k decodes, the predicted window k+1
 * is copied to the device on a second HIP stream.  hbam_split_next fills `out` (device
 * columns, valid until the next call on the stream's context) with the next window's
 * records and returns 1, returns 0 once the split is exhausted, <0 on a library error;
 * out->status != HBAM_OK (never HBAM_EMORE) is the exception nextKeyValue raises after
 * out->n_records records, and ends the stream. */
typedef struct hbam_split_stream hbam_split_stream;
hbam_split_stream* hbam_split_open(hbam_ctx* ctx, const uint8_t* file, uint64_t file_len,
                              uint64_t v_start, uint64_t v_end, int32_t n_ref,
                              uint64_t window_bytes);
/* Split-local streamed read (BAMRecordReader.java:128-143 reads only the blocks the split touches,
 * through FSDataInputStream.seek, util/WrapSeekable.java:42-87): the caller's read(user, offset,
 * len, dst) fills dst with file bytes [offset, offset + len) and returns the bytes read (> 0; a
 * positioned read such as FSDataInputStream.read(long, byte[], int, int) or pread).  Only bytes
 * from v_start's block to a bound past v_end's block are read (at most (v_end >> 16) + 192 KiB
 * unless a record runs longer), each at most once: the windows' overlap is re-used from the
 * previous window's pinned staging.  Same output as hbam_split_open on the whole file.
 * hbam_split_read_bytes: the bytes requested from `read` so far. */
typedef int64_t (*hbam_read_fn)(void* user, uint64_t offset, uint64_t len, uint8_t* dst);
hbam_split_stream* hbam_split_open_reader(hbam_ctx* ctx, hbam_read_fn read, void* user, uint64_t file_len,
                                     uint64_t v_start, uint64_t v_end, int32_t n_ref,
                                     uint64_t window_bytes);
int hbam_split_next(hbam_split_stream* s, hbam_columns* out);
/* bytes copied host->device and the copies' wall time (ms) so far */
int hbam_split_stats(const hbam_split_stream* s, uint64_t* h2d_bytes, double* h2d_ms, uint64_t* windows);
uint64_t hbam_split_read_bytes(const hbam_split_stream* s);
void hbam_split_close(hbam_split_stream* s);
/* hbam_records_to_host into the split stream's own pinned staging: valid until the next call on
 * this stream or hbam_split_close, whatever other streams of the same context do (the drop-in
 * readers: several BAMRecordReaders may share one context). */
int hbam_split_records_to_host(hbam_split_stream* s, const hbam_columns* dev, hbam_columns* host);
void hbam_free_host_columns(hbam_columns* host);
void hbam_release_columns(hbam_ctx* ctx, hbam_columns* dev);

/* ---- BAMSplitGuesser.guessNextBAMRecordStart (BAMSplitGuesser.java:109-212) -------
 * Returns the virtual offset of the guessed record, or `end`.  `file` is the whole file
 * (host or device).  *err = exception escaping the guesser (HBAM_OK normally). */
int64_t hbam_guess_bam_record_start(hbam_ctx* ctx, const uint8_t* file, int on_device,
                                    uint64_t file_len, int64_t beg, int64_t end, int32_t n_ref,
                                    int32_t* err);
/* batched guesses: k independent [beg[i], end[i]) ranges (one guesser per range). */
int hbam_guess_batch(hbam_ctx* ctx, const uint8_t* file, int on_device, uint64_t file_len,
                     const int64_t* beg, const int64_t* end, uint64_t k, int32_t n_ref,
                     int64_t* out, int32_t* err);

/* Windowed guesses: the bytes guessNextBAMRecordStart reads are the window
 * file[beg, beg + min((int)(end-beg), 262139)) cut at the end of the file
 * (BAMSplitGuesser.java:114-125; hbam_guess_window_len gives its length), so a client that
 * does not hold the file (a JVM computing getSplits over HDFS) gathers those k windows and
 * passes them concatenated: window i = windows[win_off[i], win_off[i+1]) (win_off: host,
 * k+1 entries, win_off[0] = 0; a length other than hbam_guess_window_len -> HBAM_EINVAL).
 * Same results as hbam_guess_batch over the whole file.  hbam_guess_batch itself stages only
 * these windows when `file` is on the host. */
uint64_t hbam_guess_window_len(uint64_t file_len, int64_t beg, int64_t end);
int hbam_guess_windows(hbam_ctx* ctx, const uint8_t* windows, int on_device, const uint64_t* win_off,
                       uint64_t file_len, const int64_t* beg, const int64_t* end, uint64_t k,
                       int32_t n_ref, int64_t* out, int32_t* err);

/* ---- BGZFSplitGuesser.guessNextBGZFBlockStart (util/BGZFSplitGuesser.java:51-92) ---
 * The guesser reads one window of min((int)(end-beg), 131069) bytes at beg (:62-63):
 * hbam_guess_bgzf_window takes that window alone (wlen = hbam_guess_bgzf_window_len). */
int64_t hbam_guess_bgzf_block_start(hbam_ctx* ctx, const uint8_t* file, int on_device,
                                    uint64_t file_len, int64_t beg, int64_t end, int32_t* err);
uint64_t hbam_guess_bgzf_window_len(uint64_t file_len, int64_t beg, int64_t end);
int64_t hbam_guess_bgzf_window(hbam_ctx* ctx, const uint8_t* window, int on_device, uint64_t wlen,
                               uint64_t file_len, int64_t beg, int64_t end, int32_t* err);

/* ---- BAMInputFormat.getSplits for one file (BAMInputFormat.java:76-103,163-224):
 * Hadoop FileSplits [beg[i], end[i]) -> FileVirtualSplits.  Returns the number of
 * virtual splits, or a negative code ("no reads in first split" -> HBAM_EIO).
 * hbam_probabilistic_splits_windows: the same from the file's first head_len bytes (host; the
 * BAM header — HBAM_ETRUNC: too short, read more) and the guess windows of the n FileSplits
 * (as hbam_guess_windows), for a client that reads only those bytes. */
int64_t hbam_probabilistic_splits(hbam_ctx* ctx, const uint8_t* file, int on_device,
                                  uint64_t file_len, const uint64_t* beg, const uint64_t* end,
                                  uint64_t n, uint64_t* v_start, uint64_t* v_end);
int64_t hbam_probabilistic_splits_windows(hbam_ctx* ctx, const uint8_t* head, uint64_t head_len,
                                          const uint8_t* windows, int on_device, const uint64_t* win_off,
                                          uint64_t file_len, const uint64_t* beg, const uint64_t* end,
                                          uint64_t n, uint64_t* v_start, uint64_t* v_end);

/* ---- Sort plugin path (Sort.java:84-188, SortReducer 191-205) ------
 * hbam_sort_keys: stable sort of n LongWritable keys (signed i64, Hadoop's comparator) on
 * the device; replaces the MapReduce shuffle sort of Sort's map output.  Ties keep input
 * order, so over one split's decode (voffset order) the result is ordered by (key, voffset).
 * keys (device, i64[n]) is not modified; perm (device, u32[n]) receives the source index of
 * each output position; keys_out (device, i64[n], may be NULL) the sorted keys.  n < 2^32.
 * Timing: total_ms = device time, n_blocks = radix passes run. */
int hbam_sort_keys(hbam_ctx* ctx, const int64_t* keys, uint64_t n, int64_t* keys_out,
                   uint32_t* perm);
/* hbam_gather_records: SAMRecordWritable.write (block_size + record bytes, SAMRecordWritable
 * .java:62-63) of records perm[0..n) (perm NULL = identity) from an inflated stream (ubuf,
 * rec_off, block_size: a decoded split's columns, or a received exchange buffer) into out,
 * packed; out_off (device, u64[n+1]) gets the exclusive scan of lengths.  out == NULL: size
 * query (total_bytes only).  All pointers device pointers except total_bytes (host). */
int hbam_gather_records(hbam_ctx* ctx, const uint8_t* ubuf, const uint64_t* rec_off,
                        const int32_t* block_size, const uint32_t* perm, uint64_t n, uint8_t* out,
                        uint64_t out_cap, uint64_t* out_off, uint64_t* total_bytes);
/* ---- Sort plugin, one rank's steps (Sort.java:131-170, SortRecordReader :279-295) ----------
 * A sorted run: records in (key, input order) order with their voffsets, block sizes and packed
 * SAMRecordWritable payloads (block_size field + record, SAMRecordWritable.java:62-63).  All
 * pointers are caller-owned device buffers (hbam_device_alloc): call with payload == NULL
 * first to get n and payload_bytes, then with key[n], voffset[n], block_size[n],
 * offsets[n+1] (payload offsets) and payload[payload_bytes].  A Java host drives the plugin as
 *   decode (hbam_decode_split) -> hbam_sort_split -> hbam_sort_partition with the
 *   TotalOrderPartitioner split points -> its own transport of each partition's slice ->
 *   hbam_sort_received on the concatenation of what it received (in source order).
 * Ties keep input order, so a run is ordered by (key, file order): the documented tie-break. */
typedef struct hbam_sorted_run {
  uint64_t n;
  uint64_t payload_bytes;
  int64_t* key;
  int64_t* voffset;
  int32_t* block_size;
  uint64_t* offsets;
  uint8_t* payload;
} hbam_sorted_run;
/* device buffer of `bytes` bytes followed by 64 more readable bytes, so it may be passed back as a
 * device-resident input (the 64-byte rule above); free with hbam_device_free */
int hbam_device_alloc(hbam_ctx* ctx, uint64_t bytes, void** dev_out);
/* the records of a decoded split (device columns) as a sorted run */
int hbam_sort_split(hbam_ctx* ctx, const hbam_columns* dv, hbam_sorted_run* out);
/* TotalOrderPartitioner (Sort.java:149) over a sorted run: partition k (0 <= k < nparts) holds
 * the keys in (split_points[k-1], split_points[k]] (host array of nparts-1 signed keys);
 * rec_bounds / byte_bounds (host, nparts+1) get each partition's record and payload ranges. */
int hbam_sort_partition(hbam_ctx* ctx, const hbam_sorted_run* run, const int64_t* split_points,
                        uint32_t nparts, uint64_t* rec_bounds, uint64_t* byte_bounds);
/* Multi-input Sort (Sort.java:111-113 + SortRecordReader.nextKeyValue :279-295): when the inputs'
 * sequence dictionaries differ, Utils.correctSAMRecordForMerging (cli/Utils.java:286-313) maps
 * every record of input i onto the merged dictionary.  hbam_merge_remap does it on the device
 * over a decoded split (dv, modified in place): refID -> ref_map[refID] (host, n_in entries =
 * the input's dictionary size; -1 stays -1), next refID likewise for paired reads (flag 0x1),
 * in the columns and in the record bytes, and the key recomputed (BAMRecordReader.getKey) where
 * refID changed.  *bad_record = the first record whose new index lies outside its own input's
 * dictionary (htsjdk resolves setReferenceIndex against the record's header: the reference
 * throws IllegalArgumentException there), else UINT64_MAX.  Run it before hbam_sort_split. */
int hbam_merge_remap(hbam_ctx* ctx, hbam_columns* dv, const int32_t* ref_map, int32_t n_in,
                     uint64_t* bad_record);
/* Multi-input Sort, continued: Utils.correctSAMRecordForMerging's program-group / read-group
 * rewrite (cli/Utils.java:314-324) when SamFileHeaderMerger reports ID collisions.  Over a decoded
 * split of input h (dv, after hbam_merge_remap): every record carrying the tag gets
 * setAttribute(tag, getProgramGroupId(h, value)) — for RG too (the reference's quirk: RG values are
 * looked up in the PROGRAM-group table) — and is re-encoded as BAMRecordCodec.encode writes a record
 * whose attributes changed (integer tags re-typed, odd sequence pad nibble zeroed, absent qualities
 * 0xFF, bin 0 when unplaced; restated from htsjdk 1.131, parity unpinned).  `table` (host) holds, for
 * PG then RG: u8 mode (0 no collisions of that kind: untouched; 1 translate; 2 h has no @PG record:
 * NullPointerException at the first record carrying the tag), u16 count, then `count` entries
 * {u16 old_len, old bytes, i16 new_len (-1: the value is not in the table -> tag removed; not needed:
 * an absent value is removed too), new bytes}.  On return dv's ubuf / ubuf_len / rec_off / block_size
 * point at the rewritten records (context-owned; the aux pool is not refreshed) and *status is HBAM_OK,
 * or the exception raised at record *err_record (HBAM_ENULL, HBAM_ECLASSCAST, HBAM_EFORMAT): dv then
 * holds the records before it. */
int hbam_rewrite_groups(hbam_ctx* ctx, hbam_columns* dv, const uint8_t* table, uint64_t table_len,
                        int32_t* status, uint64_t* err_record);
/* receive side: n records (device key/voffset/block_size and their packed payload, chunks in
 * source-rank order) as a sorted run */
int hbam_sort_received(hbam_ctx* ctx, const int64_t* key, const int64_t* voffset,
                       const int32_t* block_size, const uint8_t* payload, uint64_t n,
                       hbam_sorted_run* out);

/* ---- Sort plugin exchange over RCCL (Sort.java:131-170: the TotalOrderPartitioner + Hadoop
 * shuffle between map and reduce tasks; SURVEY.md §8(b) hbam_sort_multi_gpu, §8(e) steps 2-3).
 * One rank per GPU.  RCCL (librccl.so.1) is loaded on the first hbam_comm_init.
 *   rank 0: hbam_comm_unique_id(id); the job ships the 128 bytes to every rank (a Hadoop
 *           Configuration property, MPI, torch.distributed.broadcast);
 *   every rank, collectively: hbam_comm_init(ctx, id, nranks, rank, &comm);
 *   every rank, collectively: hbam_comm_split_points(ctx, comm, run, samples, sp) — regular
 *           samples of each rank's sorted keys all-gathered (ncclAllGather), the nranks-1 split
 *           points their quantiles (deterministic; the reference's RandomSampler is unseeded);
 *   every rank, collectively, twice: hbam_sort_exchange(ctx, comm, run, sp, out) — first with
 *           out->payload == NULL: the partition of `run` (hbam_sort_partition) and the count
 *           all-gather, out->n / out->payload_bytes = what this rank will receive; then with
 *           caller-owned device buffers (as hbam_sort_split): one ncclGroupStart of per-peer
 *           ncclSend / ncclRecv of keys, voffsets, block sizes and payload bytes (rank r gets
 *           the keys in (sp[r-1], sp[r]]), then hbam_sort_received on what arrived (chunks in
 *           source-rank order), so out is rank r's slice of the total order (key, file order).
 * A communicator is tied to one context (its device and stream). */
typedef struct hbam_comm hbam_comm;
#define HBAM_UNIQUE_ID_BYTES 128
int hbam_comm_unique_id(uint8_t* id_out);
int hbam_comm_init(hbam_ctx* ctx, const uint8_t* id, int32_t nranks, int32_t rank, hbam_comm** out);
void hbam_comm_destroy(hbam_comm* comm);
int hbam_comm_split_points(hbam_ctx* ctx, hbam_comm* comm, const hbam_sorted_run* run,
                           uint32_t samples_per_rank, int64_t* split_points);
int hbam_sort_exchange(hbam_ctx* ctx, hbam_comm* comm, const hbam_sorted_run* run,
                       const int64_t* split_points, hbam_sorted_run* out);

/* SplittingBAMIndexer (SplittingBAMIndexer.java:146-248, §8 f-2) from a whole-file decode
 * (dv: device columns of hbam_decode_split over [first record, len<<16|0xffff]): out (host)
 * = voffset of the first record, the voffset before every granularity-th record, then
 * file_len<<16 — the entries SplittingBAMIndex.java:50-77 reads (big-endian on disk).
 * Returns the entry count or a negative code. */
int64_t hbam_splitting_index(hbam_ctx* ctx, const hbam_columns* dv, int32_t granularity,
                             uint64_t file_len, uint64_t* out, uint64_t cap);
/* BGZFBlockIndexer.index (util/BGZFBlockIndexer.java:97-181, §8 f-3): the whole BGZF file
 * (host or device per on_device) -> out (host) = the compressed offset after every
 * granularity-th block, then the file length: the 48-bit values written big-endian as
 * [file].bgzfi and read by BGZFBlockIndex.java:50-69.  The indexer's `pos` is a Java int,
 * so entries past 2 GiB are the low 48 bits of the sign-extended wrapped value, as there.
 * Returns the entry count, HBAM_EIO where skipBlock raises IOException, or <0. */
int64_t hbam_bgzf_block_index(hbam_ctx* ctx, const uint8_t* file, int on_device, uint64_t len,
                              int32_t granularity, uint64_t* out, uint64_t cap);
/* ---- BAI index and indexed region queries (cli/plugins/Index.java:61-127 -> [htsjdk] BAMIndexer;
 * cli/plugins/View.java:164-221 -> [htsjdk] SamReader.queryOverlapping).  htsjdk is not in the
 * reference tree: the rules are restated from memory, parity unpinned (DESIGN.md lists them).
 * hbam_bai_build: the .bai of a whole-file decode (dv: device columns of hbam_decode_split over
 * [first record, len<<16|0xffff], as hbam_splitting_index takes them) serialised into `out` (host):
 * "BAI\1", n_ref, then per reference n_bin, the bins in ascending number (bin, n_chunk, (beg, end)
 * pairs in file order), the metadata pseudo-bin 37450 ((first, last offset), (records with flag 4
 * clear, set)), n_intv and the 16 KiB linear index; then u64 n_no_coor.  A record's chunk is
 * [voffset[i], voffset[i+1]); end_voffset closes the last one (the file pointer after the last
 * record, by the voffset column's rule).  The stored bin is used as it is.  Returns the byte count
 * (hbam_bai_bound is always enough; HBAM_EMORE: cap is too small), or the exception the indexer
 * raises at record *err_record: the decode's own (dv->status), HBAM_EDATA ("Unexpected reference":
 * a placed record whose refID is smaller than the previous placed record's, or outside [0, n_ref)),
 * HBAM_EINDEX (a 16 KiB window >= 32768: a position past 2^29).  Timing: total_ms = device time,
 * n_blocks = chunks written. */
uint64_t hbam_bai_bound(uint64_t n_records, int32_t n_ref);
int64_t hbam_bai_build(hbam_ctx* ctx, const hbam_columns* dv, int32_t n_ref, uint64_t end_voffset,
                       uint8_t* out, uint64_t cap, uint64_t* err_record);
/* The record filter of an indexed query over one decoded chunk range (dv: device columns): idx_out
 * (device, u32[dv->n_records]) receives, ascending, the records on ref_id with
 * start <= end && (alignment end, or start when there is none) >= beg — `contained`: start >= beg &&
 * that end <= end — in 1-based coordinates; beg <= 0 means 1, end <= 0 the end of the reference.
 * Returns the count. */
int64_t hbam_overlap_filter(hbam_ctx* ctx, const hbam_columns* dv, int32_t ref_id, int64_t beg,
                            int64_t end, int32_t contained, uint32_t* idx_out);
/* out[i] = src[perm[i]] for elem_size 4 or 8 (device pointers): carries a column (voffset,
 * block_size) through a sort permutation. */
int hbam_permute(hbam_ctx* ctx, const void* src, uint32_t elem_size, const uint32_t* perm,
                 uint64_t n, void* out);

/* ---- BAM output ---------------------------------------------------------
 * hbam_bgzf_compress: [htsjdk] BlockCompressedOutputStream under BAMRecordWriter
 * (BAMRecordWriter.java:96-111, 113-124: the writer's stream, flushed without the EOF
 * terminator) and SAMOutputPreparer.prepareForRecords (util/SAMOutputPreparer.java:58-95).
 * Cuts [src, src + n) into blocks of block_size uncompressed bytes (0: 65280, at most 65280)
 * and writes one BGZF member per block (DEFLATE on the device, CRC32, ISIZE) back to back
 * into dst.  Returns the compressed length (>= 0) or a negative hbam status; dst_cap must be
 * at least hbam_bgzf_bound(n, block_size).  The compressed bytes are not zlib's: parity is
 * on the inflated bytes (any reader of BGZF gets src back).  No terminator is written: the
 * caller appends the 28-byte EOF block where the reference does (Utils.mergeSAMInto,
 * cli/Utils.java:351-353). */
uint64_t hbam_bgzf_bound(uint64_t n, uint32_t block_size);
int64_t hbam_bgzf_compress(hbam_ctx* ctx, const uint8_t* src, int src_on_device, uint64_t n,
                           uint32_t block_size, uint8_t* dst, int dst_on_device, uint64_t dst_cap);

/* ---- read-name / CIGAR keyed consumers -------------------------------------
 * Output buffers are device memory owned by the context, valid until the next call of the same
 * entry point on that context. */
/* SummarizeRecordReader (cli/plugins/chipster/Summarize.java:664-755) over a decoded split (dv:
 * device columns of hbam_decode_split / hbam_split_next): for every record that is mapped, placed
 * and has getAlignmentStart() >= 0 (:708-709), the reference ranges of its CIGAR (parseCIGAR
 * :719-755; M/=/X runs, D/N skip) in order, each with the LongWritable key nextKeyValue sets
 * (:696-699, :714-715: getKey0(refIdx, centre of mass), then the high word kept).  status: the
 * exception nextKeyValue raises after the n ranges — the split's own (dv->status), HBAM_EREFID
 * (IllegalArgumentException: a CIGAR op code > 8) or HBAM_EINDEX (a record without a range). */
typedef struct hbam_ranges {
  uint64_t n;
  int32_t status;
  int32_t pad;
  int64_t* key;
  int32_t* beg;      /* Range.beg: 1-based, inclusive */
  int32_t* end;      /* Range.end: inclusive */
  uint8_t* rev;      /* Range.reverseStrand */
  uint32_t* record;  /* the record (index in dv) the range comes from */
} hbam_ranges;
int hbam_summarize_ranges(hbam_ctx* ctx, const hbam_columns* dv, hbam_ranges* out);
/* FixMateMapper's shuffle (cli/plugins/FixMate.java:209-221): perm (device, u32[n]) = the n records
 * at ubuf + rec_off[i] (device; a decoded split's ubuf/rec_off or a packed payload and its offsets)
 * in the order of their Text(getReadName()) keys — unsigned lexicographic, proper prefix first —
 * ties in input order (the reference leaves them unspecified). */
int hbam_name_order(hbam_ctx* ctx, const uint8_t* ubuf, const uint64_t* rec_off, uint64_t n, uint32_t* perm);
/* FixMateReducer (FixMate.java:225-277) over that shuffle order, without the combiner: the
 * reducer's writes in order.  Output k is SAMRecordWritable.write of input record src[k] — as read
 * (mate[k] == 0xffffffff: a secondary, or an unpaired primary) or after SamPairUtil.setMateInfo with
 * record mate[k] (mate fields, flags 0x8/0x20, TLEN, MQ set / MC removed, re-encoded).  The
 * reducer's quirk is kept: a primary followed only by secondaries is mated with the last of them,
 * which is written twice.  status: HBAM_EFORMAT when a mated record's attributes do not parse (the
 * job fails at output n). */
typedef struct hbam_fixmate_run {
  uint64_t n;
  uint64_t payload_bytes;
  uint64_t n_groups;   /* reduce groups (distinct read names) */
  int32_t status;
  int32_t pad;
  uint32_t* src;
  uint32_t* mate;
  uint64_t* offsets;   /* n+1 */
  uint8_t* payload;
} hbam_fixmate_run;
int hbam_fixmate(hbam_ctx* ctx, const uint8_t* ubuf, const uint64_t* rec_off, uint64_t n,
                 hbam_fixmate_run* out);

/* copy `bytes` between two device ranges (library-owned or caller-owned), ordered after the
 * context's work: how a caller keeps a call's context-owned output across the next call */
int hbam_device_copy(hbam_ctx* ctx, void* dst, const void* src, uint64_t bytes);

/* ---- the summarize plugin's reduce side and SummarySort (cli/plugins/chipster) -----------------
 * SummarizeReducer (Summarize.java:466-561) as ONE reducer over the whole job.  key / beg / end / rev
 * (device, n < 2^32 entries) are the ranges of every hbam_summarize_ranges call of the job, in
 * input order (split order, record order, range order): the caller copies them out of the
 * context-owned buffers between windows.  The call orders them by key with hbam_sort_keys (equal
 * keys keep input order: the documented tie-break, the reference leaves it unspecified), cuts the
 * stream into segments where (int)(key >>> 32) changes, and for every level L (levels: host,
 * n_levels positive int32) and strand cuts the strand's ranges of a segment into consecutive
 * groups of L.  A group is one RangeCount: beg = (int)(sumBeg / count), end = (int)(sumEnd / count)
 * with Java long sums and truncating division, count = the group's size, rid = the segment's
 * referenceID -- except that a trailing partial group flushed at a segment change carries the
 * referenceID of the NEXT segment (reduce() updates currentReferenceID before doAllSummaries(),
 * :508-511); the last segment's partial groups, flushed by cleanup(), carry their own.
 * The 2 * n_levels output streams are ordered level-major, forward strand ('f') then reverse
 * ('r'); stream k holds lines [first[k], first[k + 1]) in segment order, then group order, and its
 * text (RangeCount.toString + '\n' per line) is text[text_off[k], text_off[k + 1]).
 * sort_output != 0: each stream's lines are put in SummarySort's order first, a stable sort by
 * getKey0(rid, beg) (its sign extension kept: a negative beg makes the key's high word -1).
 * out is device memory owned by the context until the next call.  n == 0 is valid: empty streams.
 * Timing: total_ms, scan_ms = the shuffle's radix sort, walk_ms = sort_output's sorts, n_records = n,
 * n_blocks = the lines, pool_bytes = the text's bytes. */
typedef struct hbam_summary {
  uint64_t n_streams;  /* 2 * n_levels */
  uint64_t n_lines;
  uint64_t text_len;
  uint64_t n_segments;
  uint64_t* first;     /* n_streams + 1 */
  int32_t* rid;        /* n_lines each */
  int32_t* beg;
  int32_t* end;
  int32_t* count;
  uint8_t* text;
  uint64_t* text_off;  /* n_streams + 1 */
} hbam_summary;
int hbam_summarize_reduce(hbam_ctx* ctx, const int64_t* key, const int32_t* beg, const int32_t* end,
                          const uint8_t* rev, uint64_t n, const int32_t* levels, uint32_t n_levels,
                          int sort_output, hbam_summary* out);
/* SortRecordReader.nextKeyValue (chipster/SummarySort.java:240-260) over an inflated summary file
 * read as one split: text (host or device per on_device, at most 2^31 bytes, the 64-byte rule).
 * Lines are Hadoop LineReader lines: LF, a lone CR and CRLF end a line, a last line without a
 * terminator is a line, an empty line is a line.  Per line tabOne / tabTwo are its first two tabs,
 * rid = parseInt(line[0, tabOne)), pos = parseInt(line(tabOne, tabTwo)), key = getKey0(rid, pos).
 * status = the exception nextKeyValue raises after the first n lines, in file order, checked in
 * the Java's order: no tab HBAM_EINDEX (Text.decode with a negative length), rid not an int
 * HBAM_ENUMBER, no second tab HBAM_EINDEX, pos not an int HBAM_ENUMBER (a byte >= 0x80 inside a
 * field too; both choices unpinned).  start / len (without the terminator) / key cover
 * the n lines; text is the window on the device.  All owned by the context until the next call
 * that reads text.  Timing: scan_ms = structural pass, total_ms, ubuf_bytes, n_records. */
typedef struct hbam_summary_lines {
  uint64_t n;
  int32_t status;
  int32_t pad;
  const uint8_t* text;
  uint32_t* start;
  uint32_t* len;
  int64_t* key;
} hbam_summary_lines;
int hbam_summary_keys(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t len,
                      hbam_summary_lines* out);
/* SortOutputFormat's text: lines perm[0..n) of a hbam_summary_keys result (perm: device u32 indices
 * below lines->n, NULL = identity), each followed by '\n' (CRLF input comes out LF, as
 * TextOutputFormat writes it), packed into out (device); out_off (device, u64[n+1]) gets the
 * exclusive scan of the lengths + 1.  out == NULL: size query (total_bytes only), as
 * hbam_gather_records.  Timing: pools_ms, pool_bytes. */
int hbam_summary_gather_lines(hbam_ctx* ctx, const hbam_summary_lines* lines, const uint32_t* perm,
                              uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                              uint64_t* total_bytes);

/* ---- diagnostics (no reference counterpart) -----------------------------------------------
 * hbam_resolve_tokens: the LZ77 pass of the batched inflate (k_resolve) over ONE caller-built
 * token block: `io` (host, isize <= 65536 bytes) holds literal bytes with a 3-byte descriptor
 * (len-3, dist-1 little-endian) at the start of every match hole, `bitmap` (host,
 * ceil(isize/32) words) one bit per match start, tail_token/tail_dist the final match shorter
 * than 3 bytes (op | n<<16 | 1<<31, or 0).  On return `io` holds the resolved bytes and
 * *status is HBAM_OK, or HBAM_EDATA when a token points outside the block or has a distance
 * above DEFLATE's 32768 (the pass refuses such a block instead of copying from outside it). */
int hbam_resolve_tokens(hbam_ctx* ctx, uint8_t* io, uint32_t isize, const uint32_t* bitmap,
                        uint32_t tail_token, uint32_t tail_dist, int32_t* status);

/* ---- BCF over BGZF ---------------------------------------------------- */
/* BCF2Codec.readHeader: what the guesser and the record decode need from the header. */
typedef struct hbam_bcf_header {
  int32_t n_contig;       /* ##contig lines (BCF2Codec contigNames; CHROM indexes them) */
  int32_t n_sample;       /* header.getNGenotypeSamples() */
  int32_t n_dict;         /* string dictionary: PASS + FILTER/INFO/FORMAT IDs, first occurrence
                             (BCF2Utils.makeDictionary; whether htsjdk 1.131's shouldBeAddedToDictionary()
                             also admits ##ALT / ##contig lines is unverified: parity unpinned) */
  int32_t bgzf;           /* BlockCompressedInputStream.isValidFile(file) */
  uint64_t header_len;    /* uncompressed bytes of magic, l_text and the header text */
  uint64_t first_voffset; /* position of the first record: virtual offset (BGZF) or file offset */
} hbam_bcf_header;

/* BCFRecordReader output of one split (device memory owned by the context, valid until the
 * next call on it).  Record i's bytes are data[rec_off[i], +8 + l_shared + l_indiv). */
typedef struct hbam_bcf_columns {
  uint64_t n_records;
  int32_t status;       /* HBAM_OK, or the exception nextKeyValue() raises after n_records */
  int32_t pad0;
  uint64_t err_record;  /* == n_records */
  int64_t* rel;         /* BGZF: uncompressed bytes from the split start; plain: file offset */
  uint64_t* rec_off;    /* offset of the record's l_shared field in data */
  uint8_t* data;        /* the record stream: inflated blocks (BGZF) or the file window (plain) */
  uint64_t data_len;
  int64_t* key;         /* BCFRecordReader key: (long)contig index << 32 | (long)(start - 1) */
  int32_t* l_shared;
  int32_t* l_indiv;
  int32_t* chrom;
  int32_t* pos;         /* 0-based POS */
  int32_t* rlen;
  uint32_t* qual;       /* QUAL float bits */
  int32_t* n_allele_info;
  int32_t* n_fmt_sample;
} hbam_bcf_columns;

/* BCF2Codec.readHeader over the file's first `len` bytes (BGZF blocks inflated on the device).
 * HBAM_EMORE: the header runs past len.  Replaces BCFSplitGuesser.java:91-113 / BCFRecordReader
 * .initContigDict :125-133. */
int hbam_bcf_parse_header(hbam_ctx* ctx, const uint8_t* file, uint64_t len, hbam_bcf_header* out);

/* Bytes BCFSplitGuesser.guessNextBCFRecordStart(beg, end) reads (BCFSplitGuesser.java:133-145):
 * min((int)(end-beg), 2*0xffff+0xfffe) for BGZF, min(.., 0x80000) uncompressed, cut at EOF. */
uint64_t hbam_guess_bcf_window_len(uint64_t file_len, int64_t beg, int64_t end, int bgzf);

/* k guessNextBCFRecordStart calls over caller-gathered windows (window i =
 * windows[win_off[i], win_off[i+1]) = exactly hbam_guess_bcf_window_len bytes from beg[i]).
 * out[i]: virtual offset (BGZF) / file offset (plain) of the guessed record, or end[i];
 * err[i]: the exception escaping the guesser (HBAM_OK normally).  Replaces
 * BCFSplitGuesser.java:128-281 as called by VCFInputFormat.addGuessedSplits :269. */
int hbam_guess_bcf_windows(hbam_ctx* ctx, const uint8_t* windows, int on_device, const uint64_t* win_off,
                           uint64_t file_len, const int64_t* beg, const int64_t* end, uint64_t k,
                           const hbam_bcf_header* h, int64_t* out, int32_t* err);

/* BCFRecordReader over one split (BCFRecordReader.java:71-174): BGZF -> FileVirtualSplit
 * [v_start, v_end) read through BGZFLimitingStream (:177-237); plain -> FileSplit start =
 * v_start, length = v_end.  comp = file bytes [comp_base, file_len) (a BCF split reads to the
 * end of the file).  The record decode is a restated subset of htsjdk's BCF2Codec (parity
 * unpinned; oracle/hbam_oracle_bcf.c lists the rules). */
int hbam_bcf_decode_split(hbam_ctx* ctx, const uint8_t* comp, int on_device, uint64_t comp_base,
                          uint64_t comp_len, uint64_t file_len, const hbam_bcf_header* h, uint64_t v_start,
                          uint64_t v_end, hbam_bcf_columns* out);

/* ---- text VCF: VCFRecordReader (VCFRecordReader.java:72-142), the VCF half of VCFInputFormat
 * (VCFInputFormat.java:124-223) and the vcf-sort plugin (cli/plugins/VCFSort.java) ------------
 * htsjdk (AsciiLineReader, AsciiLineReaderIterator, VCFCodec) is not in the reference tree: the
 * line and decode rules are restated from memory, parity unpinned (DESIGN.md lists them).
 * Lines: a line ends at '\n'; a '\r' directly before it is not part of the line; a last line
 * without '\n' is a line; a file ending in '\n' has no empty last line; a lone '\r' is not a line
 * end here.  The header (the '#' lines through #CHROM) is parsed by the host: it passes
 * data_start (the offset of the line after #CHROM) and the contig dictionary. */

/* One slot of the contig dictionary (header.getContigLines(): ID -> ordinal, a later duplicate
 * ID overwriting the earlier one): an open-addressing table with linear probing, size a power of
 * two and at least twice the number of contigs, slot of a name = FNV-1a (32-bit, offset basis
 * 2166136261, prime 16777619) over its bytes & (size - 1).  ordinal < 0 marks an empty slot. */
typedef struct hbam_vcf_contig {
  uint32_t name_off;  /* the ID's bytes: names[name_off, name_off + name_len) */
  uint32_t name_len;
  int32_t ordinal;
} hbam_vcf_contig;

/* VCFRecordReader output of one split.  After hbam_vcf_decode_split every pointer is device memory
 * owned by the context, valid until the next hbam_vcf_decode_split on it (host = 0); after
 * hbam_vcf_columns_to_host they are host arrays owned by the caller (host = 1, text = NULL), freed
 * by hbam_vcf_release.  Line i is file bytes [line_off[i], line_off[i] + line_len[i]): the raw
 * line a Java caller hands to VCFCodec (VariantContextWritable's value). */
typedef struct hbam_vcf_columns {
  uint64_t n;          /* lines returned before `status` */
  int32_t status;      /* HBAM_OK, the exception nextKeyValue() raises after n lines, or HBAM_EMORE */
  int32_t host;
  uint64_t* line_off;  /* file offset of the line's first byte */
  uint32_t* line_len;  /* without the '\n' and a '\r' before it */
  uint32_t* tab;       /* 8 per line, relative to the line start: the ends of CHROM, POS, ID, REF, ALT,
                          QUAL, FILTER and INFO (the 8th is line_len when the line has no FORMAT) */
  int32_t* chrom;      /* contigDict ordinal of CHROM, or (int)MurmurHash3.murmurhash3(CHROM, 0) */
  int32_t* pos;        /* POS as written (1-based) */
  int32_t* ref_len;    /* bytes of REF */
  int64_t* key;        /* (long)chrom << 32 | (long)(pos - 1): the low half sign-extends, POS 0 -> -1 */
  uint8_t* text;       /* the window on the device (keep_text != 0), else NULL */
  uint64_t text_base;  /* file offset of text[0] */
  uint64_t text_len;
} hbam_vcf_columns;

/* VCFRecordReader.initialize + the nextKeyValue loop over FileSplit [start, start + length) of an
 * uncompressed VCF file of file_len bytes.  text = file bytes [text_base, text_base + text_len), a
 * window of at most 2 GiB (HBAM_EINVAL above; line offsets inside a window are 32-bit) that begins at
 * or before the reader's first byte: data_start for start == 0, else start - 1.  A device-resident
 * window that does not begin on a 16-byte boundary is read from the boundary below it (the up to 15
 * bytes before `text` must be readable, as they are inside any allocation).
 * start == 0: the lines from data_start on are candidates, positions counted from 0 (the caller has
 * raised "Empty VCF file" when there is none, :112-116).  start != 0: the reader is opened at
 * start - 1, everything through the first '\n' at or after it is discarded (:103-105) and positions
 * count from start - 1.  A candidate line is returned while one exists and its position < length
 * (:129): with start != 0 a line beginning exactly at start + length - 1 is read by no split (the
 * next one discards it); the reference's behaviour, kept.
 * Per returned line, the first failure ends the split with out->status, out->n = the lines before it:
 *   HBAM_ERUNTIME  the line begins with '#' (VCFCodec.decode returns null: NullPointerException; only
 *                  a split with start != 0 inside the header sees one);
 *   HBAM_ETRIBBLE  fewer than 8 tab-separated fields (an empty line too), or a POS that is not an
 *                  optional single '+' / '-' and one or more ASCII digits inside int32.
 * htsjdk's other validations (ID, alleles, FILTER, INFO, genotypes) are not restated.  CHROM bytes
 * are taken as UTF-16 code units of equal value.  table (host, table_size slots) and names (host,
 * names_len bytes) are the contig dictionary, copied to the device by the call.
 * out->status = HBAM_EMORE: the window ends inside the last line the split would return (or before
 * any line and before the split's bound) and before file_len; call again with a longer window.
 * Work per line is bounded by its 8th tab (by its end when it has fewer): the sample columns are
 * only read by the structural pass.  Timing: scan_ms = structural pass, walk_ms = line scan and
 * scatter, decode_ms = field pass, total_ms, ubuf_bytes = text_len, n_records = n. */
int hbam_vcf_decode_split(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t text_base,
                          uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                          uint64_t data_start, const hbam_vcf_contig* table, uint32_t table_size,
                          const uint8_t* names, uint64_t names_len, int32_t keep_text,
                          hbam_vcf_columns* out);
/* host copy of the n lines' columns (not the text: the caller holds the window) */
int hbam_vcf_columns_to_host(hbam_ctx* ctx, const hbam_vcf_columns* dev, hbam_vcf_columns* host);
/* frees a host copy's arrays; clears the struct either way */
void hbam_vcf_release(hbam_ctx* ctx, hbam_vcf_columns* cols);
/* The line writer of vcf-sort: lines perm[0..n) (device u32 indices into dv's lines, each below
 * dv->n, e.g. hbam_sort_keys' permutation of dv->key; NULL = identity) of a decode with keep_text, each
 * followed by '\n' ("\r\n" input comes out as "\n"), packed into out (device); out_off (device,
 * u64[n+1]) gets the exclusive scan of the lengths + 1.  out == NULL: size query (total_bytes
 * only), as hbam_gather_records.  Timing: pools_ms, pool_bytes. */
int hbam_vcf_gather_lines(hbam_ctx* ctx, const hbam_vcf_columns* dv, const uint32_t* perm, uint64_t n,
                          uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint64_t* total_bytes);

/* ---- SAM text: SAMRecordReader (SAMRecordReader.java) over one FileSplit of SAMInputFormat ------
 * The lines of the split become BAM records on the device (what SAMRecordWritable.write sends
 * through the shuffle: BAMRecordCodec.encode whatever the record was read from), packed into the
 * context's ubuf, and hbam_decode_split's own fixed-field and pool kernels run over them.  out is
 * a device hbam_columns owned by the context exactly as after hbam_decode_split:
 * rec_off[i + 1] == rec_off[i] + 4 + block_size[i], ubuf_len = the records' bytes, the usual slack
 * behind them; hbam_columns_to_host, hbam_records_to_host, hbam_release_columns, hbam_sort_split,
 * hbam_bai_build, hbam_summarize_ranges and hbam_fixmate take it unchanged.
 * voffset[i] is NOT a BGZF virtual offset here: it is the plain file offset of line i's first byte.
 *
 * text = file bytes [text_base, text_base + text_len): one window of at most 2 GiB (HBAM_EINVAL
 * above, before anything is read) that begins at or before the reader's first byte (data_start
 * for start == 0, else start - 1), with the alignment contract of hbam_vcf_decode_split.  The
 * host parses the header: data_start = the offset of the first byte after the last '@' line;
 * table / names = the @SQ SN dictionary, name -> ordinal, in hbam_vcf_contig's layout.
 *
 * Lines (the rules of the VCF unit): a line ends at '\n'; a '\r' directly before it is dropped; a
 * last line without '\n' is a line; there is no empty last line.
 * The split [start, start + length) returns exactly the lines whose first byte b satisfies
 * max(start, data_start) <= b < start + length (SAMRecordReader.initialize and WorkaroundingStream:
 * a split at 0 begins at data_start, any other opens at start - 1 and discards through the first
 * '\n', both read on through the first '\n' at or after start + length - 1).  Not restated:
 *   - when the stream's remaining length reaches exactly 0 at the end of one of its reader's buffer
 *     fills, the reference misses the '\n' at start + length - 1 and hands out one more line, which
 *     the next split returns too (it depends on htsjdk's buffer size);
 *   - a split with 0 < start < data_start (the reference feeds header lines to the record parser):
 *     HBAM_EUNSUPPORTED is returned.
 *   Divergence: start == 0 with length <= data_start returns no line (the reference returns the
 *   first record).
 * out->status = HBAM_EMORE as in hbam_vcf_decode_split: the window ends inside the last line the
 * split would return, before file_len; call again with a longer window.
 *
 * Per line, a subset of htsjdk's SAMLineParser and BAMRecordCodec.encode (htsjdk is not in the
 * reference tree: restated from memory, parity unpinned, DESIGN.md lists the rules).  At least 11
 * tab-separated fields; FLAG, POS, MAPQ, PNEXT, TLEN as Integer.parseInt (FLAG and MAPQ are stored
 * in 16 and 8 bits); RNAME / RNEXT through the dictionary ('*' and unknown names -1, RNEXT '='
 * RNAME's index); pos = POS - 1; CIGAR '*' or (digits op)+ over MIDNSHP=X, lengths below 2^28; SEQ
 * '*' or bytes of "=ACMGRSVTWYHKDBN" in either case, '.' read as N, packed high nibble first; QUAL
 * '*' (l_seq bytes of 0xff) or SEQ's length of bytes - 33; bin = reg2bin(pos, end), end = pos + the
 * CIGAR's reference length, pos + 1 when that is not positive or the read is unmapped (POS 0 gives
 * 4680).  Tags XX:T:value: A; Z (bytes + NUL); i written with the narrowest type in htsjdk's order
 * (I above int32, i above 65535, S above 32767, s above 255, C above 127, c down to -128, s down
 * to -32768, i below); B:<cCsSiIf>,v,... (B, the subtype, an int32 count, the values); f and B:f
 * correctly rounded to the nearest float32, ties to even, on this domain: [+-]? digits [. digits]
 * ([eE][+-]? digits)?, at most 9 significant digits once leading and trailing zeros are dropped,
 * and a decimal exponent in [-20, 20] once those digits are read as an integer (zero with any
 * exponent); other float text is HBAM_EUNSUPPORTED.
 * The first failing record ends the split: status, err_record = n_records = its index.
 *   HBAM_EUNSUPPORTED  an H tag, a read name longer than 254 bytes, more than 65535 CIGAR ops, float
 *                      text outside the domain;
 *   HBAM_EFORMAT       (SAMFormatException) fewer than 11 fields, a non-numeric or out-of-range
 *                      integer field, an empty field, a malformed CIGAR, a SEQ byte outside the
 *                      table, a QUAL whose length differs from SEQ's, a QUAL with SEQ '*', a QUAL
 *                      byte below 33, a malformed tag, an i value outside [-2^31, 2^32 - 1].
 * A line is checked in field order, the tags left to right, the SEQ and QUAL bytes last.  The
 * validations that depend on the stringency (SAMRecord.isValid, the POS / RNAME / CIGAR consistency
 * warnings) are not restated.
 *
 * key: a placed record (flag bit 4 clear, ref >= 0, POS >= 0) gets hbam_decode_split's key; any
 * other takes BAMRecordReader.getKey's second branch (:88-95; a SAM-text record has no variable
 * binary representation): MurmurHash3 chained with an int seed over the read name (chars), the
 * normalised read bases, the quality values and the CIGAR string (chars, "*" when empty), each
 * step seeded with the previous result truncated to int; Integer.MAX_VALUE << 32 | hash.  The name
 * and the CIGAR are hashed as the line writes them (a CIGAR length with leading zeros is not
 * re-rendered: unpinned).
 * Timing: scan_ms = structural pass, walk_ms = line scan, sizes and their scan, inflate_ms = the
 * text-to-BAM encode (huffman_ms = its per-line pass, resolve_ms = its SEQ / QUAL pass), decode_ms /
 * pools_ms as in hbam_decode_split, total_ms, comp_bytes = text_len, ubuf_bytes = the BAM bytes,
 * n_records. */
int hbam_sam_decode_split(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t text_base,
                          uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                          uint64_t data_start, const hbam_vcf_contig* table, uint32_t table_size,
                          const uint8_t* names, uint64_t names_len, int32_t n_ref,
                          hbam_columns* out);

/* ---- SAM text output: SAMTextWriter.writeAlignment over packed BAM records ----------------------
 * The inverse of hbam_sam_decode_split: SAMRecordWriter, the SAM half of AnySAMOutputFormat and the
 * View plugin's printing.  ubuf / rec_off = packed BAM records (block_size + record each) and their
 * offsets, u64[count + 1] with rec_off[i + 1] - rec_off[i] >= 4 + block_size of record i, and 64
 * readable bytes behind the last record: hbam_columns.ubuf / rec_off of any decode, a
 * hbam_sorted_run's payload / offsets.  Output line k is record perm[k] (device u32[n], each an index
 * into rec_off, e.g. hbam_overlap_filter's list); perm == NULL means the identity, as in
 * hbam_gather_records.  on_device == 0: ubuf and rec_off are host pointers, the library uploads them
 * with the slack, and perm must be NULL.  names / name_off are host arrays whatever on_device says:
 * the dictionary names back to back and their n_ref + 1 offsets.  n == 0 is legal and gives empty
 * text.  out's arrays are device arrays owned by the context until its next call.
 *
 * Per record, htsjdk's SAMTextWriter.writeAlignment (htsjdk is not in the reference tree: restated
 * from memory, parity unpinned, DESIGN.md lists the rules): QNAME the l_read_name - 1 name bytes; FLAG
 * decimal; RNAME the dictionary name, '*' for -1; POS (int32)(pos + 1); MAPQ; CIGAR len op over
 * MIDNSHP=X, '*' for no ops; RNEXT '=' when next_ref_id >= 0 and equal to ref_id, else the name or
 * '*'; PNEXT next_pos + 1; TLEN; SEQ through "=ACMGRSVTWYHKDBN", '*' when l_seq == 0; QUAL '*' when
 * l_seq == 0 or the first quality byte is 0xff, else each byte + 33; the tags in record order as
 * \tXX:T:value: A the raw byte, Z the bytes up to the NUL (empty: "XX:Z:"), every integer width as i
 * in decimal (C, S, I unsigned), arrays B:<sub>,v,v... (no elements: "XX:B:c"); every line ends '\n'.
 * Floats: htsjdk writes Float.toString.  The device renders a float32 (f and B:f) only where that
 * text is trivially exact: an integer value with |v| < 10^7 as "N.0", and 0.0 / -0.0.  A record
 * with any other float, or an H tag, is DEFERRED to the caller: its line is empty in text
 * (line_off[k + 1] == line_off[k]) and its output position is listed in deferred; the caller renders
 * that line and splices it in at line_off[k].  A deferred record is validated like any other.
 *
 * The first failing record ends the output: status, err_record = n_records = its output position;
 * text_len, line_off and deferred cover the lines before it.
 *   HBAM_EFORMAT  block_size < 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq, or 4 +
 *                 block_size beyond the record's rec_off slot; l_read_name == 0; l_seq < 0; a tag
 *                 that runs past the record; an unknown tag type or B subtype; a negative B count;
 *                 a Z or H without its NUL;
 *   HBAM_EREFID   (IllegalArgumentException) ref_id or next_ref_id outside [-1, n_ref); a CIGAR op
 *                 code above 8 (as hbam_summarize_ranges reports it); a quality byte above 93 when
 *                 the 0xff rule does not apply;
 *   HBAM_EUNSUPPORTED  a line of more than 2^31 - 1 bytes.
 * A record is checked in that order, the tags left to right, the quality bytes last.  Every length
 * taken from a record is checked against block_size before it is used: a malformed record gives a
 * status, never a read outside the record and the slack or a write outside text.
 * Timing: total_ms, walk_ms = sizes + scans, huffman_ms = the per-line pass (fields 1-9, tags),
 * resolve_ms = the SEQ / QUAL pass, n_records, ubuf_bytes = the text bytes. */
typedef struct hbam_sam_text {
  uint64_t n_records;
  int32_t status;
  int32_t pad;
  uint64_t err_record;
  uint64_t text_len;
  uint8_t* text;       /* device, owned by the context until the next call */
  uint64_t* line_off;  /* device u64[n+1]; line i = text[line_off[i], line_off[i+1]) with its '\n'; empty = deferred */
  uint64_t n_deferred;
  uint32_t* deferred;  /* device u32[n_deferred], ascending output positions */
} hbam_sam_text;
int hbam_sam_render(hbam_ctx* ctx, const uint8_t* ubuf, const uint64_t* rec_off, const uint32_t* perm,
                    uint64_t n, int on_device, const uint8_t* names, const uint32_t* name_off,
                    int32_t n_ref, hbam_sam_text* out);

/* ---- VCF text out of BCF records on the device: VCFRecordWriter / KeyIgnoringVCFRecordWriter
 * (VCFRecordWriter.java), VCFOutputFormat / KeyIgnoringVCFOutputFormat and the VCF half of
 * VCFSort -o out.vcf over a BCF input --------------------------------------------------------------
 * The VCF header text of a BCF file (BGZF or plain) in file[0, len), without the trailing NULs:
 * out == NULL only asks for *text_len; else at most cap bytes are written (HBAM_EINVAL when cap is
 * smaller than the text).  HBAM_EMORE and the other codes as hbam_bcf_parse_header, whose inflate
 * path this call uses. */
int hbam_bcf_header_text(hbam_ctx* ctx, const uint8_t* file, uint64_t len, uint8_t* out, uint64_t cap,
                         uint64_t* text_len);

/* What the renderer needs from the header besides hbam_bcf_header: host arrays, copied to the
 * device by the call.  The dictionary is the one hbam_bcf_parse_header counts (PASS, then the
 * FILTER / INFO / FORMAT IDs by first occurrence). */
#define HBAM_VCF_HAS_INFO 1u     /* dict_flags: the entry has an INFO line */
#define HBAM_VCF_INFO_FLAG 2u    /* ... and that line is Type=Flag or Number=0 */
#define HBAM_VCF_HAS_FORMAT 4u   /* the entry has a FORMAT line */
#define HBAM_VCF_KIND_SHIFT 4    /* (dict_flags >> 4) & 7: the FORMAT line's kind */
#define HBAM_VCF_KIND_GENERIC 0u
#define HBAM_VCF_KIND_GT 1u
#define HBAM_VCF_KIND_DP 2u
#define HBAM_VCF_KIND_GQ 3u
#define HBAM_VCF_KIND_AD 4u
#define HBAM_VCF_KIND_PL 5u
#define HBAM_VCF_KIND_FT 6u
#define HBAM_VCF_NUMBER_DOT (-1) /* dict_number: the FORMAT line's Number, a fixed integer >= 0 or one of these */
#define HBAM_VCF_NUMBER_A (-2)
#define HBAM_VCF_NUMBER_R (-3)
#define HBAM_VCF_NUMBER_G (-4)
/* The device's caps: a record above one of them is deferred to the host renderer. */
#define HBAM_VCF_MAX_INFO 64u    /* INFO pairs */
#define HBAM_VCF_MAX_FILTER 64u  /* FILTER entries */
#define HBAM_VCF_MAX_FORMAT 16u  /* genotype fields */
#define HBAM_VCF_MAX_PLOIDY 16u  /* alleles per call (the GT vector's length) */
/* Records of this many samples or more are rendered by a wave (lanes stride the samples), records
 * of fewer by one lane. */
#define HBAM_VCF_WAVE_SAMPLES 64u
typedef struct hbam_vcf_meta {
  const uint8_t* contig_names;  /* the ##contig IDs back to back */
  const uint32_t* contig_off;   /* u32[n_contig + 1] */
  const uint8_t* dict_names;    /* the dictionary strings back to back ("PASS" first) */
  const uint32_t* dict_off;     /* u32[n_dict + 1] */
  const uint32_t* dict_rank;    /* u32[n_dict]: the entry's rank in ascending String.compareTo order */
  const uint32_t* dict_flags;   /* u32[n_dict]: HBAM_VCF_* bits and the FORMAT kind */
  const int32_t* dict_number;   /* i32[n_dict]: the FORMAT line's Number */
} hbam_vcf_meta;

/* BCF2 records -> VCF text lines, the inverse direction of hbam_bcf_decode_split.  data / rec_off as
 * in hbam_bcf_columns: record i is l_shared | l_indiv | site | genotypes at data[rec_off[i]], data_len
 * the bytes of data, with 64 readable bytes behind them.  Output line k is record perm[k] (device
 * u32[n]; an index may repeat); perm == NULL is the identity.  on_device == 0: data and rec_off
 * (u64[n]) are host arrays that the library uploads with the slack, and perm must be NULL.  hdr = the
 * file's hbam_bcf_header, meta as above (host).  n == 0 is legal.  out mirrors hbam_sam_render's:
 * device arrays owned by the context until its next call; a DEFERRED line is empty in text and its
 * output position is listed in deferred; the caller renders it (hadoop_bam.vcf_text.render_record) and
 * splices it in.
 *
 * The rules (htsjdk's VCFEncoder and BCF2 decoders, restated from memory, parity unpinned):
 * Line: CHROM \t POS \t ID \t REF \t ALT \t QUAL \t FILTER \t INFO [\t FORMAT (\t sample)*] \n.
 * Typed values: descriptor and long counts as hbam_bcf_decode_split reads them.  Integer types 1 / 2 /
 *   3 have the missing value 0x80 / 0x8000 / 0x80000000; every other integer is a number, the
 *   end-of-vector codes included.  Float: 0x7F800001 is missing, anything else is the float.
 *   decodeTypedValue: count 0 is null; type 7 is the bytes with trailing NULs dropped, empty is null,
 *   and a string beginning with ',' is a list: that first comma is dropped; count 1 is the value, null
 *   when missing; count above 1 is the values with EVERY missing one dropped, all missing is null.
 *   decodeIntArray (GT, AD, PL): the values before the first missing one, none is null.
 * CHROM contigs[chrom]; POS pos + 1; ID the string, '.' when null; REF allele 0; ALT alleles 1.. joined
 *   by ',', '.' when n_allele == 1.  An allele is symbolic if it starts with '<' and ends with '>', or
 *   contains '[' or ']', or starts or ends with '.'; other alleles have a-z upper-cased.  An empty
 *   allele: HBAM_ERUNTIME.
 * QUAL: the missing float is '.'; else d = ((double)q / -10.0) * -10.0 + 0.0 written with %.2f
 *   (HALF_UP), a trailing ".00" dropped ("80", "29.60").
 * FILTER: null is '.'; else the distinct dictionary strings, ascending, joined by ';' (offset 0 prints
 *   PASS).
 * INFO, per (key, value): a key without an INFO line: HBAM_ETRIBBLE; a Flag-typed key takes the value
 *   true whatever was stored.  Ascending by key, joined by ';', '.' when there are none.  KEY alone
 *   when the text value is empty (true) or the line is Number=0, else KEY=value.  Value text: null
 *   '.', an integer decimal, a string its bytes, a list its elements joined by ',', a float through
 *   formatVCFDouble: d >= 1 %.2f; 0.01 <= d < 1 %.3f; d < 0.01 %.3e when |d| >= 1e-20, else "0.00".
 * FORMAT keys (calcVCFGenotypeKeys): every generic field non-null in some sample; GQ / DP if some
 *   sample's value is not missing; AD / PL if some sample's array is non-null; FT if some sample has
 *   it; written ascending, GT in front if some sample's GT array is non-null; an empty set with
 *   n_sample > 0 is [GT]; n_sample == 0: no FORMAT column.  A key without a FORMAT line: HBAM_ERUNTIME.
 * Per sample, header order: GT: encoded >> 1 is 0 for '.', else allele index + 1, outside [0,
 *   n_allele]: HBAM_ERUNTIME; the separator is '|' when encoded[0] & 1, else '/'; GT among the keys
 *   and this sample's array null: HBAM_ERUNTIME.  Then the other keys: DP, GQ decimal, missing '.', a
 *   vector length other than 1: HBAM_EUNSUPPORTED; AD, PL joined by ',', null '.'; generic: the INFO
 *   value text, and a null one prints '.' repeated Number times with ',' when Number is above 1
 *   (Number A = n_allele - 1, R = n_allele, a fixed integer, '.' = 1).  Trailing values made only of
 *   '.' and ',' are dropped from the sample's end; the survivors are joined by ':', after the GT when
 *   it is a key.  A genotype block whose typed values run past l_indiv: HBAM_ETRIBBLE.
 * Beyond the list (this library's choices where it is silent): a frame that runs past data_len, a
 *   typed value that runs past l_shared, a sample count other than the header's or n_allele < 1:
 *   HBAM_ETRIBBLE; CHROM outside the contigs, a dictionary offset outside the dictionary (FILTER, INFO
 *   and FORMAT keys; keys are single integers), an ID or allele that is not a string, a GT / DP / GQ /
 *   AD / PL field that is not of integer type, a second GT field, a typed value of an unknown type:
 *   HBAM_ERUNTIME.  A generic FORMAT key stored twice is written twice, in field order.  A record is
 *   checked in line order: the site left to right, the genotype fields' headers left to right, then
 *   the samples.
 * First failing record: it ends the output, as in hbam_sam_render: status, err_record = n_records =
 *   its output position; text_len, line_off and deferred cover the lines before it.
 *
 * The device renders a float only where the text is provably the rule's.  QUAL: finite, sign bit
 * clear, below 10^7, and 8q not an odd integer (there the %.2f tie meets the double round trip above).
 * INFO floats: +0.0 / -0.0 "0.00"; 0.01 <= v < 1 %.3f; 1 <= v < 10^7 %.2f; both by exact integer
 * arithmetic on mantissa and exponent, HALF_UP.  A record is DEFERRED when it has any other float; a
 * FORMAT field of float or char type, or an FT; a null generic value under Number=G; a repeated INFO
 * key (the host applies last-wins); or more INFO keys, FILTER entries, FORMAT fields or alleles per
 * call than the HBAM_VCF_MAX_* caps.  A deferred record is checked like any other.
 *
 * Every length taken from a record is checked against l_shared or l_indiv and data_len before it is
 * used: a malformed record gives a status, never a read outside the record and the slack or a write
 * outside text.  Timing: total_ms, walk_ms = the sizes passes + scans, huffman_ms = the per-line write
 * pass, resolve_ms = the per-wave write pass (records of HBAM_VCF_WAVE_SAMPLES samples or more),
 * n_records, ubuf_bytes = the text bytes. */
typedef hbam_sam_text hbam_vcf_text;
int hbam_vcf_render(hbam_ctx* ctx, const uint8_t* data, uint64_t data_len, const uint64_t* rec_off,
                    const uint32_t* perm, uint64_t n, int on_device, const hbam_bcf_header* hdr,
                    const hbam_vcf_meta* meta, hbam_vcf_text* out);

/* ---- FASTQ and QSEQ: FastqInputFormat / FastqRecordReader (FastqInputFormat.java:56-393) and
 * QseqInputFormat / QseqRecordReader (QseqInputFormat.java:58-429) over one FileSplit -------------
 * Both fill SequencedFragment values (SequencedFragment.java).  The line rule is the reference's own
 * LineReader.readLine (LineReader.java:111-173): '\n', a lone '\r' and "\r\n" all end a line, the end
 * of the file ends an unterminated one, and a line exists iff it consumes at least one byte.
 *
 * Output: device memory owned by the context, valid until the next hbam_fastq_decode_split /
 * hbam_qseq_decode_split on it (host = 0); after hbam_frag_columns_to_host host arrays owned by the
 * caller (host = 1), freed by hbam_frag_release.  Record i's key is key[key_off[i], key_off[i + 1]),
 * likewise seq and qual: the pools hold the bytes the reference hands out (qualities as Phred+33,
 * QSEQ bases with '.' as 'N').  instrument / flowcell / index are (offset, length) pairs, two u32 per
 * record, the offset relative to the window's first byte (file offset text_base); a QSEQ index
 * sequence is the raw field: its '.' -> 'N' replacement is the caller's.  present is the mask of
 * non-null fields in SequencedFragment's own bit order (Instrument 0x1, RunNumber 0x2, FlowcellId 0x4,
 * Lane 0x8, Tile 0x10, Xpos 0x20, Ypos 0x40, Read 0x80, FilterPassed 0x100, ControlNumber 0x200,
 * IndexSequence 0x400); a column whose bit is clear holds no meaning. */
#define HBAM_QUAL_SANGER 0   /* "sanger": Phred+33, checked against [33, 126] */
#define HBAM_QUAL_ILLUMINA 1 /* "illumina": Phred+64, checked against [64, 126] and rewritten as byte - 31 */
typedef struct hbam_frag_columns {
  uint64_t n;          /* records returned before `status` (records the QC filter drops are not counted) */
  int32_t status;      /* HBAM_OK, the exception next() raises after n records, or HBAM_EMORE */
  int32_t host;
  uint64_t err_pos;    /* status != HBAM_OK: the file offset the reference's position message carries */
  uint64_t first_pos;  /* getPos() before the first next(): where positionAtFirstRecord leaves the reader */
  uint64_t end_pos;    /* getPos() after the next() that ends the split (returns false, or raises) */
  uint64_t* rec_off;   /* file offset of the record's first byte */
  uint64_t* pos_after; /* getPos() after the next() that returns this record */
  uint32_t* present;
  int32_t* run;
  int32_t* lane;
  int32_t* tile;
  int32_t* xpos;
  int32_t* ypos;
  int32_t* read;
  int32_t* filter_passed; /* 0 / 1 */
  int32_t* control;
  uint32_t* instrument; /* u32[2n]: offset into the window, length */
  uint32_t* flowcell;
  uint32_t* index;
  uint64_t* key_off;   /* u64[n + 1] */
  uint64_t* seq_off;
  uint64_t* qual_off;
  uint8_t* key;
  uint8_t* seq;
  uint8_t* qual;
  uint64_t key_len;    /* bytes in each pool */
  uint64_t seq_len;
  uint64_t qual_len;
  uint64_t text_base;
} hbam_frag_columns;

/* FastqRecordReader over FileSplit [start, start + length) of an uncompressed FASTQ file of file_len
 * bytes (a gzip file: the caller inflates it and passes start = 0 and length = UINT64_MAX, the
 * reference's end = Long.MAX_VALUE).  text = file bytes [text_base, text_base + text_len), a window of
 * at most 2 GiB (HBAM_EINVAL above) with text_base <= start, under hbam_vcf_decode_split's alignment
 * contract.  encoding = HBAM_QUAL_*; filter_failed_qc != 0 drops records whose filterPassed is false.
 *
 * Positioning (positionAtFirstRecord, :158-200).  start == 0: first_pos = 0, nothing is checked.
 * start > 0: the lines are counted from byte `start` itself, and the walk ends at the first line j
 * that starts below start + length (the walk stores at most min(10000, end - start) bytes of a line:
 * from the split's end on it stores nothing and sees no '@'), whose first byte is '@' and for which either (a) line j + 2 exists, is not empty and begins with
 * '+': first_pos = the start of line j; or (b) the file has no line j + 2: the reference's loop ends
 * there too (its third read returns 0) with the reader at the start of line j + 1 (the file's length
 * when there is none), which is first_pos.  Without such a line first_pos = file_len.  The walk may
 * pass start + length; then no record is returned.
 * Records: record k is lines j + 4k .. j + 4k + 3 from first_pos.  next() returns the record at the
 * reader's position while that position < start + length, except that its filter loop reads on
 * behind a dropped record without looking at the position.  skip(1) drops the first byte untested;
 * the key is the rest of line 0, the sequence line 1, the quality line 3, each stored up to 10000
 * bytes (the rest is dropped but counted in the position); the lengths of sequence and quality are
 * not compared.  The first record that raises ends the split, status / err_pos tell how:
 *   HBAM_ERUNTIME      line 2 is empty or does not begin with '+' (err_pos = the start of line 3);
 *                      the file ends inside the record, which includes an empty line where a record
 *                      should start, directly before the end of the file ("unexpected end of file",
 *                      err_pos = file_len);
 *   HBAM_ENUMBER       a numeric group of a matching Illumina identifier lies outside int32;
 *   HBAM_ESEQFORMAT    a stored quality byte outside the encoding's range (a returned record only);
 *   HBAM_EUNSUPPORTED  an empty line where a record should start, with data behind it (skip(1) eats
 *                      the terminator and the four-line frame shifts: not restated); a key with a
 *                      byte >= 0x80 while the reader still looks for Illumina identifiers (the pattern
 *                      runs on the decoded string: not restated).
 * Illumina identifier (ILLUMINA_PATTERN, :95, matched against the whole stored key):
 * ([^:]+):(\d+):([^:]*):(\d+):(\d+):(-?\d+):(-?\d+)\s+([123]):([YN]):(\d+):(.*) with \d = ASCII digits
 * and \s = space, \t, \x0b, \f.  Records before the first whose key does not match (dropped ones
 * counted) carry all eleven fields, filter_passed = (group 9 == "N"); that record and every later
 * one carry only read, and only when the key has at least two bytes and ends in '/' and a digit.
 * HBAM_EMORE: the window ends (before file_len) inside a record the reader reads, or before the
 * positioning walk is decided; call again with a longer window.
 * Timing: scan_ms structural pass, walk_ms line starts and positioning, decode_ms the record passes,
 * pools_ms scans, compaction and pools, total_ms, ubuf_bytes = text_len, n_records, pool_bytes. */
int hbam_fastq_decode_split(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t text_base,
                            uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                            int32_t encoding, int32_t filter_failed_qc, hbam_frag_columns* out);
/* QseqRecordReader, the same arguments; the window begins at or before start - 1 (0 for start == 0).
 * Positioning (:138-157): start > 0 opens at start - 1 and drops the line read there; first_pos = the
 * start of the next line.  One line is one record, returned while the reader's position < start +
 * length (and behind a dropped record, as above).  Per line, in this order:
 *   HBAM_ERUNTIME      the line consumes 20000 bytes or more (err_pos = its start);
 *   HBAM_ESEQFORMAT    setFieldPositionsAndLengths finds other than 11 fields: its loop ends when it
 *                      reaches the line's length, so an empty line has 0 fields, the empty field
 *                      behind a trailing tab is not counted, and fields behind the 11th are ignored
 *                      (err_pos = the position after the line - the line's length, as the message);
 *   HBAM_EUNSUPPORTED  a byte >= 0x80 in fields 0-7 (Text.decode is not restated);
 *   HBAM_ENUMBER       fields 1, 2, 3, 4, 5, 7 (run, lane, tile, x, y, read) are Integer.parseInt:
 *                      [+-]? digits inside int32;
 *   HBAM_ESEQFORMAT    a quality byte (field 9) outside the encoding's range, returned records only.
 * key = fields 0-5 with their tabs as ':', ':' and field 7; filter_passed = (first byte of field 10
 * != '0'); the index sequence is null when field 6 is not empty and begins with '0'; the sequence is
 * field 8 with '.' as 'N'.  flowcell and control are never present.
 * Both positioning walks call readLine(Text, int): the int is maxLineLength (what is stored), not
 * maxBytesToConsume, so no line of a walk is cut and the positions do not depend on LineReader's
 * buffer size. */
int hbam_qseq_decode_split(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t text_base,
                           uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                           int32_t encoding, int32_t filter_failed_qc, hbam_frag_columns* out);
/* host copy of the n records' columns and the three pools */
int hbam_frag_columns_to_host(hbam_ctx* ctx, const hbam_frag_columns* dev, hbam_frag_columns* host);
/* frees a host copy's arrays; clears the struct either way */
void hbam_frag_release(hbam_ctx* ctx, hbam_frag_columns* cols);

/* ---- FASTQ and QSEQ output: FastqRecordWriter.write (FastqOutputFormat.java:94-147) and
 * QseqRecordWriter.write (QseqOutputFormat.java:100-159) over hbam_frag_columns ---------------------
 * The inverse of the two decodes above.  cols = device columns as a decode on this context left them
 * (host = 0), or a host copy (host = 1), which the library uploads into context buffers.  window =
 * the bytes the instrument / flowcell / index pairs point into, window_len < 2^32 of them, host
 * (window_on_device == 0: uploaded) or device memory at any alignment; no byte at or past window_len
 * is read.  Output record k is record perm[k] of cols (device u32[n]: a selection, a reorder,
 * duplicates allowed; device columns only); perm == NULL means records 0 .. n - 1, n <= cols->n.
 * n == 0 is legal and gives empty text.  format = HBAM_FRAG_*, encoding = HBAM_QUAL_* (of the text
 * written; the pools hold Phred+33, as the reference's SequencedFragment does).  out's arrays are
 * device arrays owned by the context until its next hbam_frag_render.
 *
 * HBAM_EINVAL (returned, nothing rendered): an unknown format, encoding or flag; perm with host
 * columns; n >= 2^32 - 1; n > cols->n without perm; host key_off / seq_off / qual_off that do not
 * ascend or leave their pool; a present host string pair that runs past window_len.  Device columns
 * are trusted to be device arrays of cols->n records with 16 readable bytes behind each pool (what a
 * decode leaves); their contents are checked per record in the sizes pass, where a perm entry >=
 * cols->n, offsets that descend or leave the pool, a length above 2^31 - 1 or a present string pair
 * past window_len ends the output there with status HBAM_EINVAL (the call returns HBAM_OK).
 *
 * FASTQ.  '@' id '\n' seq "\n+\n" qual '\n'.  With HBAM_FRAG_USE_KEY id = the record's key bytes
 * (write(key != null, ...)); otherwise makeId: instrument:run:flowcell:lane:tile:x:y, a space,
 * read:F:control:index.  A field whose present bit is clear is empty; integers as Integer.toString
 * ('-', no padding, down to -2147483648); F = 'N' when filter_passed is absent or non-zero, else 'Y';
 * control absent = "0"; index absent = empty, with HBAM_FRAG_INDEX_DOTS each '.' in it as 'N' (the
 * raw QSEQ field, see the columns above).  The strings' bytes are written as they are
 * (makeId(...).getBytes() uses the platform charset: unpinned).  HBAM_QUAL_SANGER: the quality bytes
 * verbatim, unchecked.  HBAM_QUAL_ILLUMINA: SequencedFragment.convertQuality Sanger -> Illumina
 * (SequencedFragment.java:234-247): every byte, as a signed byte, must lie in [33, 126], else
 * HBAM_ESEQFORMAT; the byte written is (uint8_t)(b + 31), so 96 .. 126 leave as 127 .. 157 unchecked.
 * The reference has then already written "@id\nseq\n+\n": partial_len is that length and those bytes
 * stand at text[text_len, text_len + partial_len).
 *
 * QSEQ.  instrument \t run \t lane \t tile \t x \t y \t index \t read \t seq \t qual \t filter \n.
 * index: absent or empty = "0", else 'N' as '.' (a '.' stays, with or without INDEX_DOTS); seq: 'N'
 * as '.'; filter '1' when absent or non-zero, else '0'; key, flowcell and control are not written.
 * HBAM_QUAL_SANGER: quality verbatim.  HBAM_QUAL_ILLUMINA: b + 31; a result above 126 (b > 95) is
 * HBAM_ERUNTIME, there is no lower bound.  The reference works on the decoded String: a byte >= 0x80
 * in seq or qual is HBAM_EUNSUPPORTED (Text decode / encode are not restated), which wins over
 * HBAM_ERUNTIME in the same record.  Nothing of a failing record is written: partial_len = 0.
 *
 * The first failing record in output order ends the call: status, err_record = n_records = its
 * output position, text_len = line_off[n_records]; the records before it stand.
 * Timing: total_ms, walk_ms = sizes + scan, huffman_ms = the per-record pass (id line / leading
 * fields, separators, filter), resolve_ms = the sequence / quality pass, n_records, ubuf_bytes = the
 * text bytes. */
#define HBAM_FRAG_FASTQ 0
#define HBAM_FRAG_QSEQ 1
#define HBAM_FRAG_USE_KEY 1u    /* FASTQ: the id line is '@' + the record's key */
#define HBAM_FRAG_INDEX_DOTS 2u /* the index column is a raw QSEQ field: '.' reads as 'N' */
typedef struct hbam_frag_text {
  uint64_t n_records;   /* complete records in text */
  int32_t status;       /* HBAM_OK or what write() raises at record err_record */
  int32_t pad;
  uint64_t err_record;  /* output position */
  uint64_t text_len;    /* bytes of the n_records complete records */
  uint64_t partial_len; /* bytes of record err_record the reference's stream already holds when it throws */
  uint8_t* text;        /* device, owned by the context until the next render */
  uint64_t* line_off;   /* device u64[n_records + 1] */
} hbam_frag_text;
int hbam_frag_render(hbam_ctx* ctx, const hbam_frag_columns* cols, const uint8_t* window, int window_on_device,
                     uint64_t window_len, const uint32_t* perm, uint64_t n, int32_t format, int32_t encoding,
                     uint32_t flags, hbam_frag_text* out);

/* ---- FASTA: FastaInputFormat.getSplits (FastaInputFormat.java:59-144) and FastaRecordReader
 * (:146-361) over one FileSplit, filling ReferenceFragment values (ReferenceFragment.java) ----------
 * The line rule is LineReader.readLine's, as for FASTQ and QSEQ above.
 *
 * hbam_fasta_sections: the file offsets (text_base + the position in the window) of every byte '>'
 * of text[0, text_len), ascending, into the host array out_off[cap]; *n = their count.  getSplits
 * starts a section at every '>' wherever it stands in a line: with p0 < p1 < ... < pm over the whole
 * file its splits are (p_i, p_{i+1} - 1 - p_i) and (p_m, file_len - p_m), and (0, file_len) without
 * any.  text is host or device memory at any alignment under hbam_vcf_decode_split's window contract,
 * at most 2 GiB (HBAM_EINVAL above).  cap too small: HBAM_EMORE, *n is the count and nothing is
 * written (cap = 0 with out_off = NULL is the size query).  Timing: scan_ms the byte scan, walk_ms
 * scan + scatter, total_ms, ubuf_bytes = text_len, n_records = *n. */
int hbam_fasta_sections(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t text_base, uint64_t text_len,
                        uint64_t* out_off, uint64_t cap, uint64_t* n);

/* Output of hbam_fasta_decode_split: device memory owned by the context, valid until its next
 * hbam_fasta_decode_split (host = 0); after hbam_fasta_columns_to_host host arrays owned by the
 * caller (host = 1), freed by hbam_fasta_release.  Record i's key is key[key_off[i], key_off[i + 1]),
 * its sequence seq[seq_off[i], seq_off[i + 1]).  The indexSequence every record carries is the
 * window's bytes [index_off, index_off + index_len), tabs kept. */
typedef struct hbam_fasta_columns {
  uint64_t n;          /* records returned before `status` */
  int32_t status;      /* HBAM_OK, the exception the constructor (n = 0) or next() raises, or HBAM_EMORE */
  int32_t host;
  uint64_t err_pos;    /* HBAM_ERUNTIME: the file offset of the line the message names */
  uint64_t first_pos;  /* getPos() before the first next(): the byte after the header line */
  uint64_t end_pos;    /* getPos() after the next() that ends the split (returns false, or raises) */
  uint64_t* rec_off;   /* file offset of the line's first byte */
  uint64_t* pos_after; /* getPos() after the next() that returns this record */
  int32_t* position;   /* ReferenceFragment.position */
  uint32_t* line_len;  /* the line's own bytes: seq[seq_off[i], seq_off[i] + line_len[i]) is the clean line */
  uint64_t* key_off;   /* u64[n + 1] */
  uint64_t* seq_off;
  uint8_t* key;
  uint8_t* seq;
  uint64_t key_len;    /* bytes in each pool */
  uint64_t seq_len;
  uint32_t index_off;  /* relative to the window's first byte (file offset text_base) */
  uint32_t index_len;
  uint64_t text_base;
} hbam_fasta_columns;

/* FastaRecordReader over FileSplit [start, start + length) of an uncompressed FASTA file of file_len
 * bytes.  text = file bytes [text_base, text_base + text_len), a window of at most 2 GiB (HBAM_EINVAL
 * above) with text_base <= start, under hbam_vcf_decode_split's alignment contract.  (A compressed
 * file never reaches this call: its reader has no indexSequence and its first non-empty line raises
 * NullPointerException, which the caller answers on the host.)
 *
 * Constructor (positionAtFirstRecord, :207-232): the line at `start` is read whole; its first
 * min(20000, length) content bytes are stored.  indexSequence = the stored bytes without the first,
 * which is dropped untested.  first_pos = start + the bytes the line consumes.  n = 0 and
 *   HBAM_EINDEX        nothing stored (substring(1, 0)): length == 0, an empty line, the end of the file;
 *   HBAM_EUNSUPPORTED  a stored byte >= 0x80 (Text.toString / String.getBytes are not restated).
 * next (:322-339): every line that starts below start + length is a record, empty lines and later
 * '>' lines included, and is read to its own end; the end of the file ends the split.  A line that
 * consumes 20000 bytes or more is HBAM_ERUNTIME (err_pos = its start, end_pos = the byte behind
 * it); the records before it stand.  position = 1 + (rec_off - first_pos) in Java int arithmetic:
 * it counts bytes consumed, terminators included.  key = indexSequence + Integer.toString(position)
 * with every '\t' as ':'.
 * Sequence (scanFastaLine, :359) = line.getBytes() whole, the backing array of a Hadoop 1.2.1 Text
 * that also held the header line and every earlier line: clear() keeps the array, append()
 * reallocates to exactly the needed size only when it is too small (restated from upstream, unpinned).
 * With L_-1 the stored header length ('>' included) and L_k the length of data line k, record k has
 * cap_k = max(L_-1, L_0 .. L_k) bytes: byte c is the line's own for c < L_k, else byte c of line j,
 * the largest j in [-1, k) with L_j > c.
 * HBAM_EMORE: the window ends (before file_len) inside the header line or a line the reader reads;
 * call again with a longer window.  HBAM_ENOMEM (returned): a pool does not fit device memory.
 * Timing: scan_ms structural pass, walk_ms line starts and the header line, decode_ms the record
 * pass, maxima and offsets, pools_ms the two pools, total_ms, ubuf_bytes = text_len, n_records,
 * pool_bytes. */
int hbam_fasta_decode_split(hbam_ctx* ctx, const uint8_t* text, int on_device, uint64_t text_base,
                            uint64_t text_len, uint64_t file_len, uint64_t start, uint64_t length,
                            hbam_fasta_columns* out);
/* host copy of the n records' columns and the two pools */
int hbam_fasta_columns_to_host(hbam_ctx* ctx, const hbam_fasta_columns* dev, hbam_fasta_columns* host);
/* frees a host copy's arrays; clears the struct either way */
void hbam_fasta_release(hbam_ctx* ctx, hbam_fasta_columns* cols);

#ifdef __cplusplus
}
#endif
#endif
