/*
 * ffq.h -- C ABI of libffq_hip.so: the MI355X (gfx950) FASTQ buffer-scan path.
 *
 * This is the drop-in boundary for the hot path of lgautier/fastq-and-furious
 * (reference checkout: /root/reference).  Every entry point names the
 * reference interface it replaces (file:line).  Plain pointers and sizes only;
 * no torch / Python types.  The reference-side binding a maintainer would add
 * is shown in INTEGRATION.md.
 *
 * Coordinates.  The reference scanners work on one `bytes` buffer; the
 * iterator prepends a b'\n' sentinel to the stream (fastqandfurious.py:245)
 * and compensates with globaloffset = -1 (:242).  All scan entry points take
 *   sentinel = 0  the n_bytes ARE the buffer the scanner sees, or
 *   sentinel = 1  the buffer is b'\n' + bytes, without the copy,
 * and work in BUFFER coordinates (index into that buffer).  `add` is added to
 * every emitted position (entryfunc_abspos' globaloffset, :186-195), so
 * sentinel = 1, add = -1 yields absolute file offsets.
 *
 * Errors.  Functions return FFQ_OK (0) or a negative FFQ_E_* code;
 * ffq_last_error() gives the text for the calling thread.  There is no CPU
 * fallback anywhere in this library: without a usable gfx950 device the
 * context cannot be created and every compute call fails.
 */
#ifndef FFQ_H
#define FFQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFQ_ABI_VERSION 12

/* scanner status codes -- identical to the reference's module constants
 * (_fastqandfurious.c:7-15,254-262; fastqandfurious.py:19-27)             */
#define FFQ_INVALID                 (-1)
#define FFQ_POS_HEAD_BEG            0   /* MISSING_SEQHEADER_BEGIN */
#define FFQ_POS_HEAD_END            1   /* MISSING_SEQHEADER_END   */
#define FFQ_POS_SEQ_BEG             2   /* MISSING_SEQ_BEG         */
#define FFQ_POS_SEQ_END             3   /* MISSING_SEQ_END         */
#define FFQ_POS_QUAL_BEG            4   /* MISSING_QUAL_BEGIN      */
#define FFQ_POS_QUAL_END            5   /* MISSING_QUAL_END        */
#define FFQ_COMPLETE                6
#define FFQ_MISSING_QUALHEADER_END  7

/* end states of a record chain = the exits of readfastq_iter's loop
 * (fastqandfurious.py:256-279)                                            */
#define FFQ_END_OK              0   /* eof, stream ended cleanly (:257-258, :264-266) */
#define FFQ_END_REFILL          1   /* !eof, entry incomplete: caller refills (:274-279) */
#define FFQ_END_ERR_FINAL_QUAL  2   /* 'Incomplete final quality string at byte' (:262) */
#define FFQ_END_ERR_INCOMPLETE  3   /* 'Incomplete entry at byte %i' (:269)            */
#define FFQ_END_ERR_INVALID     4   /* 'Entry is invalid at byte %i' (:272; at eof the
                                       reference loops forever, we report this instead) */
/* ... and of a pair of streams (ffq_pair_next) */
#define FFQ_END_ERR_PAIR_COUNT  5   /* one file of a pair holds more records than the other */
#define FFQ_END_ERR_PAIR_NAMES  6   /* the i-th records of the two files are not mates      */

/* return codes */
#define FFQ_OK               0
#define FFQ_E_NODEVICE      (-1)
#define FFQ_E_HIP           (-2)
#define FFQ_E_ARG           (-3)
#define FFQ_E_NOMEM         (-4)
#define FFQ_E_TABLE_FULL    (-5)   /* more records than table_cap: n_records holds the need */
#define FFQ_E_INTERNAL      (-6)
#define FFQ_E_TIMEOUT       (-7)   /* a shard step's watchdog: ffq_last_error names the stage and the ranks */

/* flags for the scan calls */
#define FFQ_F_DECODE_QUAL   1u     /* also emit Phred-decoded qualities (value added = qual_add) */
#define FFQ_F_FORCE_SERIAL  2u     /* debugging/tests: use the single-wave chain walker */
#define FFQ_F_FORCE_RANKED  4u     /* debugging/tests: use the list-ranking tier */
#define FFQ_F_FORCE_GENERAL 64u    /* debugging/tests: skip the four-line fast path (the general chain kernels and, through
                                      dense regions, the window walker take plain four-line input too)             */
#define FFQ_F_POLL_RESULT   8u     /* completion is signalled through the result block the last kernel
                                      writes into host-mapped memory (ffq_scan_wait polls a word of it)
                                      instead of through an event recorded behind that kernel: one stream
                                      marker less per scan (~3 us of idle GPU); ms_chain / ms_total are
                                      not measured then.  Ignored with FFQ_F_DECODE_QUAL.              */

#define FFQ_F_SINGLE_PASS  16u     /* with FFQ_F_DECODE_QUAL: the caller accepts the decoded qualities WITH GAPS instead of packed --
                                      the bytes of record i are d_qual[d_qoff[i] : d_qoff[i] + (pos5 - pos4)], contiguous and in
                                      file order, but there may be gaps between records (d_qoff[i + 1] - d_qoff[i] is NOT a
                                      length; n_qual_bytes = where the last record's bytes end).  On plain four-line input the
                                      line-index pass itself then writes them (csrc/ffq_fused.h; res.path 6) and the input is
                                      read ONCE -- HBM traffic 1.0 x the algorithmic bytes instead of 1.5 x -- in one of two
                                      layouts, by the room the caller gives:
                                        qual_cap >= FFQ_SEG_STRIDE per 16 KiB tile of the buffer (rounded up): SEGMENTED, every
                                          tile owns that many bytes of d_qual and packs the quality lines that start in it
                                          there; lines up to 512 bytes behind a tile's end (reads of a few hundred bases);
                                        qual_cap >= FFQ_INPLACE_STRIDE per tile: also IN PLACE, d_qoff[i] = the offset pos4 has
                                          in d_buf -- lines of any length (long reads); taken when the segmented pass refuses
                                          the buffer for its shape, and first from then on (until ffq_ctx_forget).
                                      Records of ANY other layout -- WRAPPED ones, whose quality lines are known only behind
                                      the record chain -- decode in one pass as well with FFQ_INPLACE_STRIDE bytes per tile
                                      (round 6): a scan that starts on the general kernels (a context that has met such input
                                      remembers it) has its index pass write EVERY byte of the buffer decoded at its own
                                      offset, d_qoff[i] = the offset pos4 has in d_buf (res.path | FFQ_PATH_IN_PLACE); an
                                      embedded newline of a wrapped quality comes out as '\n' + qual_add, as the reference's
                                      slice + arrayadd_b give it (_fastqandfurious.c:129, doc/user-guide.rst:126-141).
                                      Less room -- or four-line input the single pass cannot vouch for (a quality line longer
                                      than its read, text in front of the first record), or the first scan of a context that
                                      only finds out on the way that its input is not four-line -- and the two passes run: the
                                      output is packed (a special case of the same contract).                                */
#define FFQ_SEG_STRIDE     8704
#define FFQ_INPLACE_STRIDE 16384
#define FFQ_PATH_IN_PLACE  8       /* ffq_scan_result.path bit: see there */
#define FFQ_F_NO_TIMING    32u     /* with FFQ_F_POLL_RESULT: no timing marks around the line-index kernel either (ms_index is
                                      0 for this scan): the front then holds no stream marker at all.  Where the library itself
                                      can prove that the order does not matter it also dispatches the index kernel without a
                                      barrier, so that it starts while the previous scan's last, one-workgroup kernel is still
                                      running: only when the last thing enqueued on the context's stream is the front of another
                                      scan (a context sharing the stream; anything else the library enqueues there -- copies, the
                                      stream front end's event waits, table utilities -- ends that, and so does handing the stream
                                      out through ffq_ctx_stream), and none of that scan's outputs overlaps the bytes this one
                                      reads.  The caller vouches for nothing.  A host that times every n-th scan loses nothing but
                                      the marks' idle microseconds on the others.                                            */

typedef struct ffq_ctx ffq_ctx;

typedef struct ffq_scan_result {
    int64_t n_records;      /* rows of the chain (all of them, even if > table_cap)      */
    int64_t n_qual_bytes;   /* total decoded quality bytes (FFQ_F_DECODE_QUAL)           */
    int64_t end_offset;     /* buffer coordinate where the last, unsuccessful search
                               started: the iterator's `offset` at exit (:254, :275-277) */
    int64_t last_pos[6];    /* posbuffer as the last scanner call left it (+add applied
                               to entries != -1); for FFQ_END_OK after the final-record
                               rule, the final record's row                              */
    int32_t last_status;    /* status of that last call                                   */
    int32_t end_state;      /* FFQ_END_*                                                  */
    int32_t path;           /* 3 = four-line fast path, 6 = the same with the Phred decode done by
                               the index pass itself (one pass over the input), 0 = general chain
                               kernels, 2 = the same with the dense LDS budget, 5 = list ranking
                               over the "\n@" matches (long records), 1 = serial walker;
                               | FFQ_PATH_IN_PLACE (8, on 0 / 2 / 5 / 1): the index pass of that
                               scan also decoded every byte in place -- records of any layout,
                               one pass (FFQ_F_SINGLE_PASS)                                */
    int32_t retries;        /* internal re-runs (line-index pool growth)                  */
    int64_t n_lines;        /* newline count seen by the line-index kernel                */
    float   ms_index;       /* device time of the line-index kernel (hipEvent)            */
    float   ms_chain;       /* device time of chain summary + resolve + emit kernels      */
    float   ms_decode;      /* device time of the quality decode kernel                   */
    float   ms_total;       /* device time of the whole call                              */
} ffq_scan_result;

/* ---- library / context ------------------------------------------------ */
int         ffq_abi_version(void);
/* Hash (16 hex digits) of the sources this binary was compiled from: csrc/ and include/ of this
 * repository, computed by build.py and baked in at compile time.  The Python host recomputes it
 * from the tree and rebuilds (or refuses to run) when the two differ, so a stale in-tree .so
 * cannot stand in for the sources.                                                             */
const char *ffq_build_id(void);
const char *ffq_last_error(void);
int         ffq_device_count(void);
/* device = HIP ordinal.  Fails (FFQ_E_NODEVICE) if it is not a gfx950 part. */
int         ffq_ctx_create(int device, ffq_ctx **out);
/* A second context on the same HIP streams as `parent` (own scratch): work submitted
 * through either context executes in submission order.  With ffq_scan_submit/_wait this
 * lets a host queue the next batch behind the current one (no idle GPU between batches).
 * Destroy it before the parent.                                                        */
int         ffq_ctx_create_shared(ffq_ctx *parent, ffq_ctx **out);
void        ffq_ctx_destroy(ffq_ctx *ctx);
/* Pre-size the per-context scratch (line index, group summaries) for buffers
 * of up to max_bytes so that no allocation happens inside a timed scan.     */
int         ffq_ctx_reserve(ffq_ctx *ctx, int64_t max_bytes);
/* A context remembers whether its recent input was plain four-line FASTQ and
 * then starts the following scans with the kernels that fit (results are the
 * same either way).  This forgets that history.                             */
void        ffq_ctx_forget(ffq_ctx *ctx);
/* The HIP stream all of this context's work is enqueued on (hipStream_t): a stream of the
 * context's own, created hipStreamNonBlocking -- it does NOT wait for the legacy default stream or
 * for any other stream.  Whatever fills d_buf (or clears the output buffers) on another stream must
 * be complete, or ordered in front of this stream by the caller (an event recorded there and waited
 * for here), before a scan is submitted.                                                           */
void       *ffq_ctx_stream(ffq_ctx *ctx);

/* ---- memory plumbing (so a ctypes host needs nothing else) ------------ */
int ffq_dev_alloc(ffq_ctx *ctx, int64_t bytes, void **dptr);
int ffq_dev_free(ffq_ctx *ctx, void *dptr);
int ffq_pinned_alloc(int64_t bytes, void **hptr);
int ffq_pinned_free(void *hptr);
int ffq_copy_h2d(ffq_ctx *ctx, void *dptr, const void *hptr, int64_t bytes, int async);
int ffq_copy_d2h(ffq_ctx *ctx, void *hptr, const void *dptr, int64_t bytes, int async);
int ffq_sync(ffq_ctx *ctx);

/* ---- the hot path ------------------------------------------------------
 * Record chain over one device-resident buffer.  Replaces the per-record
 * loop `status = entrypos(buf, offset, posbuffer); yield entryfunc(...)` of
 * readfastq_iter (fastqandfurious.py:251-279) with the C extension's scanner
 * semantics (_fastqandfurious.c:25-153) for every record of the buffer at
 * once.  d_buf must be 16-byte aligned.
 *
 *   offset      buffer coordinate where the first "\n@" search starts
 *   eof         nonzero: apply the iterator's end-of-stream rules (:256-270)
 *   d_table     device int64[table_cap][6]: pos0..pos5 per record, + add
 *   d_qual      device int8[qual_cap] or NULL: with FFQ_F_DECODE_QUAL the
 *               bytes buf[pos4:pos5] + qual_add of every record, packed
 *               (arrayadd_b, _fastqandfurious.c:161-185; usage
 *               doc/user-guide.rst:130-141)
 *   d_qoff      device int64[table_cap+1] or NULL: start of record i in d_qual
 * Blocks until the result is known.                                        */
int ffq_scan_device(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes,
                    int sentinel, int64_t offset, int eof, int64_t add,
                    uint32_t flags, int qual_add,
                    int64_t *d_table, int64_t table_cap,
                    int8_t *d_qual, int64_t qual_cap, int64_t *d_qoff,
                    ffq_scan_result *res);

/* The same in two halves: ffq_scan_submit enqueues the kernels and returns at once;
 * ffq_scan_wait blocks, applies the fallbacks if the input needs them, and fills `res`.
 * One scan may be pending per context.                                                 */
int ffq_scan_submit(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes,
                    int sentinel, int64_t offset, int eof, int64_t add,
                    uint32_t flags, int qual_add,
                    int64_t *d_table, int64_t table_cap,
                    int8_t *d_qual, int64_t qual_cap, int64_t *d_qoff);
int ffq_scan_wait(ffq_ctx *ctx, ffq_scan_result *res);

/* Same over a host buffer: pinned staging + hipMemcpyAsync in, kernels, rows
 * (and qualities) copied back.  h_table: int64[table_cap][6].              */
int ffq_scan_host(ffq_ctx *ctx, const uint8_t *h_buf, int64_t n_bytes,
                  int sentinel, int64_t offset, int eof, int64_t add,
                  uint32_t flags, int qual_add,
                  int64_t *h_table, int64_t table_cap,
                  int8_t *h_qual, int64_t qual_cap, int64_t *h_qoff,
                  ffq_scan_result *res);

/* One scanner call: entrypos(blob, offset, posbuffer) -> status
 * (_fastqandfurious.c:25-153).  Host buffers; pos receives 6 x int64.       */
int ffq_entrypos(ffq_ctx *ctx, const uint8_t *h_buf, int64_t len, int64_t offset,
                 int64_t *pos, int *status);

/* arrayadd_b(a, value): int8[i] += value in place, wrapping
 * (_fastqandfurious.c:161-185).  _device: a is device memory.               */
int ffq_arrayadd_b_device(ffq_ctx *ctx, int8_t *d_a, int64_t n, int value);
int ffq_arrayadd_b(ffq_ctx *ctx, int8_t *h_a, int64_t n, int value);
/* arrayadd_q(a, value): int64[i] += value in place, wrapping
 * (_fastqandfurious.c:193-217).                                             */
int ffq_arrayadd_q_device(ffq_ctx *ctx, int64_t *d_a, int64_t n, int64_t value);
int ffq_arrayadd_q(ffq_ctx *ctx, int64_t *h_a, int64_t n, int64_t value);

/* First row i of a device offset table (rows sorted by record) with
 * d_table[i][col] >= value; n_rows if none.  Used to cut a shard's rows out of
 * a table that also covers its halo (multi-GPU byte-range sharding).        */
int ffq_table_lower_bound(ffq_ctx *ctx, const int64_t *d_table, int64_t n_rows, int col,
                          int64_t value, int64_t *idx);

/* The rows of a byte-range shard inside the table of its scan: out = {i0, i1, pos0[i0],
 * pos0[i1], pos5[i0 - 1], pos5[i1 - 1]} with i0 / i1 the first rows whose pos0 (column 0) is
 * >= lo / >= hi (n_rows if none; the positions are -1 then), and pos5 of the rows right in
 * front of them (-1 if there is none): the record chain found row i searching from
 * pos5[i - 1] - 1 (fastqandfurious.py:254), which is where a neighbour shard re-enters the
 * chain.  One launch, one host wait.                                          */
int ffq_table_cut(ffq_ctx *ctx, const int64_t *d_table, int64_t n_rows, int64_t lo, int64_t hi,
                  int64_t out[6]);

/* Rows of a device offset table whose sequence length pos3 - pos2 lies in
 * [min_len, max_len], in order, written to d_out (n_rows rows of room; not
 * d_table itself); *n_out = rows kept.  The length filter of the reference's
 * user guide (doc/user-guide.rst:153-180) evaluated on the table, before any
 * per-record object exists: filtering reads is deleting rows (:199-204).    */
int ffq_table_select_seqlen(ffq_ctx *ctx, const int64_t *d_table, int64_t n_rows, int64_t min_len,
                            int64_t max_len, int64_t *d_out, int64_t *n_out);
/* ... with d_idx[i] = the ordinal in d_table of kept row i (n_rows entries of room; NULL: none): what a host
 * that owes one item per ORIGINAL row -- the guide's loop sees None for a dropped record (:166-170) -- puts the
 * kept ones back by.                                                                                       */
int ffq_table_select_seqlen_idx(ffq_ctx *ctx, const int64_t *d_table, int64_t n_rows, int64_t min_len,
                                int64_t max_len, int64_t *d_out, int64_t *d_idx, int64_t *n_out);

/* One component of every row of a device offset table as a packed stream + CSR offsets: byte j of
 * row i's component is d_out[d_off[i] + j] = buf[pos[col_begin] + begin_shift + j] + value_add,
 * up to pos[col_end].  This is what an entryfunc that builds only one part of an entry returns
 * (doc/user-guide.rst:153-180: buf[posarray[2]:posarray[3]]; the header as entryfunc cuts it,
 * fastqandfurious.py:161-171: col_begin 0, begin_shift 1, col_end 1), evaluated for the whole
 * table on the device; with columns 4 / 5 and value_add = -33 it is the Phred decode
 * (doc/user-guide.rst:206-214).  d_buf / n_bytes / sentinel / add: the buffer the rows were
 * scanned from and the `add` of that scan (rows - add are buffer coordinates).  d_off: n_rows + 1
 * entries.  *n_out_bytes = bytes of the stream; FFQ_E_TABLE_FULL if out_cap is smaller (nothing
 * is written past out_cap: d_off is complete, d_out holds the first out_cap bytes of the stream;
 * d_out may be NULL if out_cap is 0 -- the sizing call).  After ffq_table_select_seqlen this is the
 * user guide's length-filter entryfunc in two calls.
 * Rows are independent: any order, repeated, overlapping, written by hand.  A component is EMPTY
 * (d_off[i + 1] == d_off[i]) if its end does not lie above its beginning (pos[col_end] <=
 * pos[col_begin] + begin_shift: rows of length 0 as a trim leaves them, however many in a row; the
 * -1, -1 of a FASTA row; a row of negative length) or if it does not lie inside the buffer, i.e.
 * unless 0 <= pos[col_begin] + begin_shift - add - sentinel and pos[col_end] - add - sentinel <=
 * n_bytes (with sentinel, coordinate 0 is the virtual "\n": never read).  A component partly outside
 * is empty as a whole; no byte outside [d_buf, d_buf + n_bytes) is read.  value_add is added to
 * every byte modulo 256 (arrayadd_b's wrap-around, _fastqandfurious.c:161-185; only its low 8 bits
 * count) and the sum is stored as int8: value_add = -33 turns '!' into 0 and the byte 0x10 into -17.
 * d_out: no alignment asked.                                                                   */
int ffq_table_gather_column(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                            const int64_t *d_table, int64_t n_rows, int col_begin, int begin_shift,
                            int col_end, int value_add, int8_t *d_out, int64_t out_cap, int64_t *d_off,
                            int64_t *n_out_bytes);

/* Quality trimming by MODIFYING rows -- the other thing the user guide's table of indices is for ("trimming either end
 * of the read could be done by ... modifying the values in a table of indices", doc/user-guide.rst:196-204) -- with the
 * running-sum rule of BWA's and cutadapt's -q.  For one row, q[0..n) = buf[pos4:pos5] (unsigned bytes):
 *     start = 0; stop = n
 *     s = 0; best = 0; for i = 0 .. n-1:  s += cutoff_front - (q[i] - qual_base); if s < 0: break;
 *                                         if s > best: best = s, start = i + 1          (5' end)
 *     s = 0; best = 0; for i = n-1 .. 0:  s += cutoff_back  - (q[i] - qual_base); if s < 0: break;
 *                                         if s > best: best = s, stop = i               (3' end, independent of the 5')
 *     if start >= stop: start = stop = 0                    (trimmed away: the header stays, the length is 0)
 * and the row becomes pos0, pos1, pos2 + start, pos2 + stop, pos4 + start, pos4 + stop.  Ties keep the first maximum; a
 * cutoff of 0 leaves an end alone unless bytes lie below qual_base; the sums are carried in 64 bits.  A row is trimmed
 * only if pos2..pos5 - add are all >= 0, pos2 <= pos3 and pos4 <= pos5 lie inside the buffer (with sentinel, coordinate
 * 0 is the virtual "\n"), pos3 - pos2 == pos5 - pos4 and no quality byte is "\n"; every other row -- wrapped records,
 * FASTA rows (-1), rows that point outside the buffer -- is copied unchanged and counted as skipped; no byte outside
 * [d_buf, d_buf + n_bytes) is read.  d_buf / n_bytes / sentinel / add: as for ffq_table_gather_column.  d_out: n_rows
 * rows; it MAY be d_table (rows are independent).  Both tables 16-byte aligned.  stats = {rows changed, bases removed
 * (front + back, summed over the rows), rows skipped}.  FFQ_E_ARG: cutoffs outside 0..127, qual_base outside 0..255, a
 * scan pending on the context.  One host wait.  After it, ffq_table_select_seqlen drops what became too short and
 * ffq_table_gather_column returns the trimmed sequence or (value_add = -33) the trimmed, decoded quality.             */
int ffq_table_trim_quality(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                           const int64_t *d_table, int64_t n_rows, int qual_base, int cutoff_front, int cutoff_back,
                           int64_t *d_out, int64_t stats[3]);

/* 3' adapter trimming by MODIFYING rows: what `cutadapt -a ADAPTER --no-indels -e E -O O` does, with E = err_permille /
 * 1000 and O = min_overlap.  For one row, seq[0..n) = buf[pos2:pos3], ad[0..m) the adapter (1 <= m <= 64), min_overlap in
 * 1..m, err_permille in 0..1000:
 *     cut = n
 *     for p = 0 .. n - min_overlap:                 (leftmost first; no candidate if n < min_overlap)
 *         ov = min(m, n - p)                        (a full copy inside the read, or a prefix of the adapter at its 3' end)
 *         mm = #{ j < ov : ad[j] != 'N' and seq[p + j] != ad[j] }
 *         if mm <= (ov * err_permille) / 1000:      (integer division)
 *             cut = p; break
 * and the row becomes pos0, pos1, pos2, pos2 + cut, pos4, pos4 + cut.  Bytes are compared as they are (a lower-case read
 * does not match an upper-case adapter); 'N' (0x4E) in the adapter matches any byte, 'N' in the read only an 'N' of the
 * adapter; mismatches only, no insertions or deletions.  ONE DIFFERENCE from cutadapt: of several qualifying positions the
 * LEFTMOST is taken, not the best-scoring one.  A row is trimmed only if pos2..pos5 - add are all >= 0, pos2 <= pos3 and
 * pos4 <= pos5 lie inside the buffer (with sentinel, coordinate 0 is the virtual "\n": never read), pos3 - pos2 == pos5 -
 * pos4 and no byte of the whole sequence buf[pos2:pos3] is "\n" (a wrapped record is left alone even when a hit lies in
 * front of its newline); every other row is copied unchanged and counted as skipped; a row of length 0 is eligible,
 * unchanged and not skipped.  No byte outside [d_buf, d_buf + n_bytes) and outside the row's own checked sequence range is
 * read.  adapter: HOST memory.  d_buf / n_bytes / sentinel / add: as for ffq_table_gather_column.  d_out: n_rows rows; it
 * MAY be d_table.  Both tables 16-byte aligned.  stats = {rows changed, bases removed, rows skipped}.  FFQ_E_ARG:
 * adapter_len outside 1..64, min_overlap outside 1..adapter_len, err_permille outside 0..1000, a scan pending on the
 * context.  One host wait.  Run it behind ffq_table_trim_quality (cutadapt's order: -q first).  Not done: 5' and anchored
 * adapters, indels, several adapters per call.  (Adapters found by the overlap of a pair's mates: ffq_table_pair_overlap.) */
int ffq_table_trim_adapter(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                           const int64_t *d_table, int64_t n_rows, const uint8_t *adapter, int adapter_len,
                           int err_permille, int min_overlap, int64_t *d_out, int64_t stats[3]);

/* Poly-G / poly-X tail trimming by MODIFYING rows: what `fastp --trim_poly_g` / `--trim_poly_x` are for.  A two-colour
 * instrument reads "no signal" as G, so a fragment shorter than the read ends in a run of high-quality G that the quality trim
 * cannot see.  For one row, seq[0..n) = buf[pos2:pos3]; cls(byte) = 0 / 1 / 2 / 3 for A a / C c / G g / T t and 4 for anything
 * else (the classes of ffq_table_stats; a byte that is no base -- N -- matches nothing); the walk position i = 0, 1, ... is
 * byte seq[n-1-i]; allowed(i) = min(5, (i + 1) / 8), integer division; the set of bases is S = {base} for base 0..3 (poly-G:
 * base 2) and S = {0, 1, 2, 3} for FFQ_POLY_ANY (poly-X); min_len in 2..65535:
 *     mm[b] = 0, hit[b] = 0, last[b] = -1   for b in S;   stop = n
 *     for i = 0 .. n-1:
 *         k = cls(seq[n-1-i])
 *         t[b] = mm[b] + (k != b)                          for b in S
 *         if i >= min_len - 1 and t[b] > allowed(i) for EVERY b in S:  stop = i; break
 *         mm = t;  if k in S: hit[k] += 1, last[k] = i
 *     if stop < min_len: the row is unchanged
 *     else: b* = the b in S with the most hits (ties: the lowest class); new length len' = n - 1 - last[b*]
 * and the row becomes pos0, pos1, pos2, pos2 + len', pos4, pos4 + len'.  Inside the first min_len - 1 positions nothing stops
 * the walk.  A row that is trimmed had exactly one base still passing at stop - 1 -- two bases mismatch each other at every
 * position, so they cannot both be within `allowed` -- and the tie rule never decides a trimmed row.  The tail is cut back to
 * its deepest exact b*: mismatching bytes at the inner edge of the tail stay on the read.  A read that is all tail goes to
 * length 0.  This is fastp's rule in spirit -- one mismatch allowed per eight positions, at most five; min_len is its
 * poly_g_min_len / poly_x_min_len (default 10) -- but it has NOT been checked against fastp's source, which was not at hand.
 * One known departure: N never matches, whereas fastp's poly-X counts N for every base.  Eligibility is
 * ffq_table_trim_adapter's: pos2..pos5 - add all >= 0, in order, inside the buffer (with sentinel, coordinate 0 is the
 * virtual "\n": never read), pos3 - pos2 == pos5 - pos4 and no byte of the whole sequence is "\n" (a wrapped record is left
 * alone even when its last line is all G); every other row is copied unchanged and counted as skipped; a row of length 0 is
 * eligible and unchanged.  No byte outside the row's own checked sequence range is read; the quality line is never read.
 * d_buf / n_bytes / sentinel / add: as for ffq_table_gather_column.  d_out: n_rows rows; it MAY be d_table.  Both tables
 * 16-byte aligned.  stats = {rows changed, bases removed, rows skipped}.  FFQ_E_ARG: base outside 0..3 and not FFQ_POLY_ANY,
 * min_len outside 2..65535, misaligned tables, a scan pending on the context.  One host wait.  Not done: wrapped records, 5'
 * tails, cutadapt's --nextseq-trim quality weighting.                                                                  */
#define FFQ_POLY_ANY (-1)
int ffq_table_trim_poly(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                        const int64_t *d_table, int64_t n_rows, int base, int min_len, int64_t *d_out, int64_t stats[3]);

/* Fixed trims and sliding-window quality cutting of both read ends by MODIFYING rows: what fastp's -f / -t / -b and its
 * --cut_front / --cut_right / --cut_tail (-5 / -r / -3), Trimmomatic's SLIDINGWINDOW and cutadapt's -u / -l are for.  Run it
 * in FRONT of every other trim (fastp's order).  For one row, q[0..n) = buf[pos4:pos5] as unsigned bytes; v[i] = (int)q[i] -
 * qual_base, which may be negative; S(i, W) = v[i] + ... + v[i+W-1].  Sums are 32 bits inside a window, positions 64 bits.
 * trim_front, trim_tail, keep_len: each >= 0.  Three windows, FRONT, RIGHT and TAIL: each with `window` in 0..64 (0: off) and
 * `quality` in 1..93:
 *     a = min(trim_front, n);  b = n - min(trim_tail, n - a)             (fixed trims)
 *     if keep_len > 0 and b - a > keep_len:  b = a + keep_len            (the 3' end gives way)
 *     front (if on and b > a):   W = min(window, b - a);  T = quality * W
 *         s = the smallest i in a .. b-W with S(i, W) >= T;   none: the read goes to length 0, done
 *         a = s;  while v[a] < quality: a += 1              (a window that passes holds such a base: this ends inside it)
 *     right (if on and b > a):   W = min(window, b - a);  T = quality * W
 *         s = the smallest i in a .. b-W with S(i, W) < T;    none: nothing happens
 *         b' = s;  while b' < s + W and v[b'] >= quality: b' += 1;   b = b'  (the good bases at the head of the bad window stay)
 *     tail (if on and b > a):    W = min(window, b - a);  T = quality * W
 *         e = the largest j in a+W .. b with S(j-W, W) >= T;   none: length 0, done
 *         b = e;  while v[b-1] < quality: b -= 1
 *     if a >= b: a = b = 0
 * and the row becomes pos0, pos1, pos2 + a, pos2 + b, pos4 + a, pos4 + b.  A range shorter than the window is judged as one
 * window of its own length (W = min(...)); a stage that meets an empty range does nothing.  "Mean >= quality" is compared as
 * sum >= quality * W, with no division.  Positions behind the last full window of `right` are never judged: that is what
 * `tail` is for.  This is fastp's -5 / -r / -3 and Trimmomatic's SLIDINGWINDOW in spirit, but it has NOT been checked
 * against either source, which was not at hand.  Eligibility is ffq_table_trim_quality's: pos2..pos5 - add all >= 0, in
 * order, inside the buffer (with sentinel, coordinate 0 is the virtual "\n": never read), pos3 - pos2 == pos5 - pos4 and no
 * byte of the WHOLE quality line is "\n" -- the bytes the fixed trims take off included; every other row is copied unchanged
 * and counted as skipped; a row of length 0 is eligible and unchanged.  No byte outside the row's own checked quality range
 * is read; the sequence line is never read.  d_buf / n_bytes / sentinel / add: as for ffq_table_gather_column.  d_out:
 * n_rows rows; it MAY be d_table.  Both tables 16-byte aligned.  stats = {rows changed, bases removed, rows skipped}.
 * FFQ_E_ARG: a window above 64, a quality outside 1..93 on a window that is on, negative counts, qual_base outside 0..255,
 * all of it off, misaligned tables, a scan pending on the context.  One host wait.  Not done: windows above 64, wrapped
 * records, push-down through readfastq_iter, per-stage counts.                                                          */
typedef struct ffq_ends_rules {
    int32_t trim_front, trim_tail, keep_len, qual_base, front_window, front_quality, right_window, right_quality, tail_window,
        tail_quality;
} ffq_ends_rules;
int ffq_table_trim_ends(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                        const int64_t *d_table, int64_t n_rows, const ffq_ends_rules *rules, int64_t *d_out, int64_t stats[3]);

/* Per-cycle base and quality statistics of a table, counted on the device: what the QC report of fastp / FastQC is made
 * of.  d_stats: DEVICE memory, 16-byte aligned, FFQ_STATS_WORDS(C) uint64 words with C = max_cycles; overwritten
 * (accumulate == 0, whatever they held) or added to (accumulate != 0).  For one eligible row, seq = buf[pos2:pos3], q =
 * buf[pos4:pos5], n = len(seq), v[i] = clamp(q[i] - qual_base, 0, 95), cls[i] = 0 / 1 / 2 / 3 for A a / C c / G g / T t
 * and 4 for every other byte:
 *     words 0..7            head: [0] rows counted, [1] rows skipped, [2] bases (sum of n), [3] bases at cycles >= C,
 *                                 [4] sum of v over all bases, [5] bases of class 1 or 2 (GC), [6] bases of class 4, [7] 0
 *     8 + c*5 + b           cycle_base[c][b]: for every i < min(n, C): [i][cls[i]] += 1
 *     8 + 5C + c*96 + v     cycle_qual[c][v]: for every i < min(n, C): [i][v[i]] += 1
 *     8 + 101C + l          len_hist[l], l in 0..C: [min(n, C)] += 1 (the last bin is "C or longer")
 *     8 + 102C + 1 + m      readq_hist[m]: if n > 0: [(sum of v) / n] += 1 (integer division)
 *     8 + 102C + 97 + g     gc_hist[g]: if n > 0: [(100 * gc) / n] += 1, gc = bases of class 1 or 2
 * Bases at cycles >= C count in the head and in the two per-read histograms, not in the per-cycle arrays.  A row is
 * ELIGIBLE if pos2..pos5 - add are all >= 0, pos2 <= pos3 and pos4 <= pos5 lie inside the buffer (with sentinel, coordinate
 * 0 is the virtual "\n": never read), pos3 - pos2 == pos5 - pos4 and no byte of the sequence or of the quality is "\n" (a
 * wrapped record); every other row adds 1 to head[1] and nothing else; a row of length 0 counts in head[0] and len_hist[0]
 * only.  Rows are independent: any order, repeated, overlapping.  No byte outside [d_buf, d_buf + n_bytes) is read.  All
 * sums are integers added with integer atomics: the result does not depend on the order of anything.  d_buf / n_bytes /
 * sentinel / add: as for ffq_table_gather_column.  head: HOST memory; non-NULL: one host wait, words 0..7 of d_stats as they
 * stand after this call; NULL: the call only enqueues on the context's stream.  n_rows == 0 is valid (accumulate == 0: the
 * block is zeroed).  FFQ_E_ARG: max_cycles outside 1..FFQ_STATS_MAX_CYCLES, qual_base outside 0..255, d_stats NULL or
 * misaligned, a scan pending on the context.                                                                          */
#define FFQ_STATS_QBINS      96     /* quality value v = clamp(byte - qual_base, 0, 95) */
#define FFQ_STATS_GCBINS     101
#define FFQ_STATS_HEAD       8
#define FFQ_STATS_MAX_CYCLES 4096
#define FFQ_STATS_WORDS(C)   (8 + (int64_t)(C) * 101 + ((C) + 1) + 96 + 101)
int ffq_table_stats(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                    const int64_t *d_table, int64_t n_rows, int qual_base, int max_cycles,
                    int accumulate, uint64_t *d_stats, int64_t head[FFQ_STATS_HEAD]);

/* Rows kept or dropped for what is IN the read: cutadapt's --max-n and --max-ee, fastp's -n, -e, -q / -u and -y, evaluated
 * on the table with the length filter in front of them.  The content rules: */
typedef struct ffq_content_rules {
    int32_t qual_base;            /* 0..255 */
    int32_t max_n;                /* -1: off */
    int32_t min_mean_qual;        /* 0: off; 1..95 */
    int32_t qualified_qual;       /* 0..95: a base with v < this is "unqualified" */
    int32_t max_unqualified_pct;  /* -1: off; 0..100 */
    int32_t min_complexity_pct;   /* 0: off; 1..100 */
    int64_t max_ee_micro;         /* -1: off; expected errors in millionths */
} ffq_content_rules;
/* For one row, seq = buf[pos2:pos3], q = buf[pos4:pos5], n = len(seq), v[i] = clamp(q[i] - qual_base, 0, 95) -- the v of
 * ffq_table_stats.  The quantities a row is judged by:
 *     nN = number of i with seq[i] equal to 'N' or 'n'
 *     sv = sum of v[i]
 *     u  = number of i with v[i] < qualified_qual
 *     ee = sum of FFQ_EE_MICRO[v[i]]
 *     d  = number of i < n - 1 with seq[i] != seq[i + 1]
 * FFQ_EE_MICRO[v] = floor(1e6 * 10^(-v/10) + 0.5), 96 constants written into the source as literals (no entry lies closer
 * than 0.001 to a rounding boundary): ffq_ee_micro_table() returns them.
 * A row gets a VERDICT: the first rule that fails, in this order, or 0 for kept.
 *     1 length           pos3 - pos2 < min_len or > max_len: the test of ffq_table_select_seqlen, on any row, eligible or
 *                        not.  A row that fails it has none of its bytes read.
 *     2 N                max_n >= 0 and nN > max_n
 *     3 mean quality     min_mean_qual > 0 and sv < min_mean_qual * n
 *     4 unqualified      max_unqualified_pct >= 0 and 100 * u > max_unqualified_pct * n
 *     5 expected errors  max_ee_micro >= 0 and ee > max_ee_micro
 *     6 complexity       min_complexity_pct > 0 and n >= 2 and 100 * d < min_complexity_pct * (n - 1)
 * Rules 2 to 6 apply only to rows that are ELIGIBLE exactly as for ffq_table_stats (positions inside the buffer and in
 * order, the two lines of one length, no line with bytes in it beginning at the sentinel's coordinate 0, no "\n" in the
 * sequence or the quality).  Every other row -- wrapped records, FASTA rows (-1), rows that point outside the buffer -- is
 * judged by its length alone and counted as "not judged".  A row of length 0 is eligible and passes rules 2 to 6.
 * Everything is integer arithmetic; sv, ee and the products are carried in 64 bits wherever a row can be long.  No byte
 * outside [d_buf, d_buf + n_bytes) is read.  Rows are independent: any order, repeated, overlapping, written by hand.
 *
 * ffq_table_select_reads writes the kept rows (verdict 0), in order, to d_out (n_rows rows of room; not d_table; both
 * tables 16-byte aligned) and d_idx[i] = the ordinal in d_table of kept row i (NULL: none); *n_out = rows kept.  counts:
 *     [0] rows kept; [1]..[6] rows dropped by rule 1..6; [0..6] sum to n_rows and *n_out == counts[0];
 *     [7] rows not judged by content although a content rule is on; they are also counted in [0] or [1].  As a row dropped
 *         by its length has no byte read, such a row counts in [7] only if its POSITIONS already make it ineligible (a
 *         wrapped record that is too short or too long counts in [1] alone).
 * d_buf / n_bytes / sentinel / add: as for ffq_table_gather_column.  rules == NULL, or rules with every content rule off:
 * the call is ffq_table_select_seqlen_idx -- the same launches, rows and d_idx, no kernel reads the buffer and d_buf may be
 * NULL; only counts[0] and [1] are non-zero.  n_rows == 0 is valid.  One host wait.  FFQ_E_ARG: a field outside its range, a
 * scan pending on the context, d_buf NULL with n_bytes > 0 while a content rule is on.  Paired-end files:
 * ffq_table_select_pairs below.  Not done: the fraction form of --max-n.                                               */
#define FFQ_FILTER_COUNTS 8
int ffq_table_select_reads(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                           const int64_t *d_table, int64_t n_rows, int64_t min_len, int64_t max_len,
                           const ffq_content_rules *rules, int64_t *d_out, int64_t *d_idx, int64_t *n_out,
                           int64_t counts[FFQ_FILTER_COUNTS]);
const uint32_t *ffq_ee_micro_table(void);

/* ---- paired-end files: two tables whose i-th rows are mates (R1.fq / R2.fq) ------------------------------------------
 * A mate's buffer and table, as every table pass takes them (d_buf / n_bytes / sentinel / add: as for
 * ffq_table_gather_column; d_table 16-byte aligned).                                                                  */
typedef struct ffq_table_view { const uint8_t *d_buf; int64_t n_bytes; int32_t sentinel; int64_t add; const int64_t *d_table; } ffq_table_view;
#define FFQ_PAIR_ANY   0   /* drop the pair if either mate fails (cutadapt --pair-filter=any, its default) */
#define FFQ_PAIR_BOTH  1   /* drop it only if both fail                                                  */
#define FFQ_PAIR_FIRST 2   /* mate 1 alone decides; mate 2 is not judged and none of its bytes is read   */
/* ffq_table_select_pairs: a pair is kept or dropped together.  Row i of m1 and row i of m2 are mates.  Each mate gets the
 * VERDICT v1 / v2 that ffq_table_select_reads would give it on its own -- the same rules in the same order, the same
 * eligibility, "a row dropped by its length has none of its bytes read" -- with its own length bounds (len_bounds = min1,
 * max1, min2, max2: cutadapt -m 30:20) and its own rules.  rules == NULL or every content rule off: that mate is judged by
 * its length alone, no kernel reads its buffer and its d_buf may be NULL.  The pair is DROPPED if
 *     FFQ_PAIR_ANY    v1 != 0 || v2 != 0
 *     FFQ_PAIR_BOTH   v1 != 0 && v2 != 0
 *     FFQ_PAIR_FIRST  v1 != 0                   (mate 2 is not judged at all)
 * Kept pairs go to d_out1 and d_out2 (n_pairs rows of room each; neither may be one of the tables; 16-byte aligned), in
 * order; d_idx[k] = the ordinal of kept pair k (NULL: none); *n_out = pairs kept.
 * hist1 / hist2: the eight counts of ffq_table_select_reads for that mate's rows judged alone, whatever became of the
 * pair ([0] rows with verdict 0, [1..6] by rule, [7] not judged by content).  FFQ_PAIR_FIRST: hist2 is all zero.
 * pairs = {kept, dropped, only mate 1 failed, only mate 2 failed, both failed}; [0] + [1] = n_pairs.  FFQ_PAIR_FIRST:
 * [2] = number of pairs with v1 != 0, [3] = [4] = 0.
 * n_pairs == 0 is valid.  One host wait.  FFQ_E_ARG: a pair_filter that is none of the three, a field of either rules out
 * of range, a scan pending on the context, d_buf NULL with n_bytes > 0 for a judged mate whose content rules are on.
 * Merging the kept pairs' mates: ffq_table_pair_merge.  Not done: interleaved input or output.                         */
int ffq_table_select_pairs(ffq_ctx *ctx, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                           const int64_t len_bounds[4] /* min1, max1, min2, max2 */,
                           const ffq_content_rules *rules1, const ffq_content_rules *rules2, int pair_filter,
                           int64_t *d_out1, int64_t *d_out2, int64_t *d_idx, int64_t *n_out,
                           int64_t hist1[FFQ_FILTER_COUNTS], int64_t hist2[FFQ_FILTER_COUNTS], int64_t pairs[5]);
/* ffq_table_pair_names: are these two files really mates?  For one row, h = buf[pos0 + 1 : pos1], the header as entryfunc
 * cuts it.  id(h) = h up to, not including, its first byte that is 0x20 (space) or 0x09 (tab); all of h if there is none.
 * If that id has at least two bytes and ends in "/1" or "/2", those two bytes go as well (an id that is exactly "/1"
 * becomes empty).  A pair is EQUAL if the two ids have the same length and the same bytes.  A pair is COMPARED if, for both
 * mates, pos0 - add >= 0, pos0 + 1 <= pos1 and the slice lies inside the buffer (it may end at its end; with sentinel,
 * coordinate 0 is the virtual "\n": never read) -- the render pass's condition on its header slice.  Every other pair (FASTA
 * rows, rows written by hand that point outside) counts as NOT COMPARED.  No byte outside either buffer is read.
 * out = {equal, different, not compared, ordinal of the first different pair or -1}.  n_pairs == 0 is valid.  One host
 * wait.  FFQ_E_ARG: a scan pending on the context, d_buf NULL with n_bytes > 0.
 * This is this library's own rule, not cutadapt's: cutadapt strips "/1" and "/2" as well as a trailing "1", "2" or "3"
 * of either id before it compares, and so accepts ids that differ in that last digit alone; here only the two-byte forms
 * go, and everything else has to match byte for byte.                                                                 */
int ffq_table_pair_names(ffq_ctx *ctx, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                         int64_t out[4] /* equal, different, not compared, ordinal of the first different pair or -1 */);

/* ffq_table_pair_overlap: the overlap of the two mates of a pair -- the insert size of every pair, and adapters cut without
 * naming them: what fastp does to paired-end reads by default.  The two mates read the same fragment from both ends; when
 * the fragment is shorter than a read, mate 1 and the reverse complement of mate 2 overlap, and what sticks out beyond the
 * overlap is adapter, whatever its sequence.  Row i of m1 and row i of m2 are mates.  For one pair:
 *     a[0..n1)  = buf1[pos2:pos3] of mate 1, b[0..n2) = buf2[pos2:pos3] of mate 2
 *     cls(x)    = the class of ffq_table_stats: 0 / 1 / 2 / 3 for A a / C c / G g / T t, 4 for every other byte
 *     rb[j]     = 3 - cls(b[n2-1-j]) if that class is < 4, else 4: the reverse complement of mate 2
 *     position i of a and j of rb MATCH if cls(a[i]) < 4 and cls(a[i]) == rb[j]; an N matches nothing, not even an N
 *
 *     if n1 < min_overlap or n2 < min_overlap: no candidate
 *     candidates o, IN THIS ORDER: 0, 1, ..., n1 - min_overlap, then -1, -2, ..., -(n2 - min_overlap)
 *         lo = max(0, o); hi = min(n1, n2 + o); ov = hi - lo              (>= min_overlap by construction)
 *         mm = #{ i in [lo, hi) : a[i] and rb[i - o] do not match }
 *         if mm <= min(max_diff, (ov * diff_permille) / 1000):            (integer division)
 *             found: o* = o; stop
 *     insert = n2 + o*          (the length of the fragment: from a's first base to rb's last)
 *     if trim and o* < 0:       c1 = min(n1, insert), c2 = min(n2, insert)   (c2 == insert always)
 *         row 1 becomes pos0, pos1, pos2, pos2 + c1, pos4, pos4 + c1; row 2 likewise with c2
 * Only o* < 0 cuts -- fastp's choice: for o* >= 0, insert < n1 can only happen when mate 2 was shortened beforehand, and
 * then a[insert:] is not known to be adapter.  THREE DIFFERENCES from fastp: the whole overlap is counted (fastp accepts a
 * candidate on its first 50 positions); N never matches; both mates are cut to min(len, insert), not to fastp's
 * overlap_len.  A consequence: bases that a 5' quality trim took off mate 2 make `insert` smaller by as many; mate 1 is then
 * cut that much short of the adapter, never beyond it.  Mismatches only, no insertions or deletions.
 * A pair is ANALYSED if both rows are eligible exactly as for ffq_table_trim_adapter (positions >= 0 and in order inside
 * the buffer, pos3 - pos2 == pos5 - pos4, the sentinel's coordinate never read, no "\n" in the whole sequence) and both
 * lengths are <= FFQ_OVERLAP_MAX_LEN.  Every other pair -- wrapped records, FASTA rows, rows written by hand that point
 * outside, long reads -- has both rows copied unchanged and counts as not analysed.  No byte outside either [d_buf, d_buf +
 * n_bytes) is read and none outside the rows' own checked sequence ranges; the quality line is never read.
 * d_out1 / d_out2: n_pairs rows each, 16-byte aligned; they MAY be the input tables (pairs are independent).  d_insert
 * (NULL: none): DEVICE memory, per pair `insert`, -1 for analysed without an overlap, -2 for not analysed.  d_hist (NULL:
 * none): DEVICE memory, 8-byte aligned, FFQ_OVERLAP_HIST_WORDS uint64: hist[insert] += 1 per pair with an overlap;
 * overwritten (accumulate == 0) or added to (accumulate != 0), as ffq_table_stats does; integer atomics only: the result
 * does not depend on the order of anything.  counts: [0] pairs analysed, [1] pairs with an overlap, [2] pairs with at least
 * one row changed, [3] bases removed from mate 1, [4] from mate 2, [5] pairs not analysed; [0] + [5] == n_pairs.
 * n_pairs == 0 is valid.  One host wait.  FFQ_E_ARG: a field out of range, rules NULL, a scan pending on the context, a
 * misaligned table, d_insert or d_hist, d_buf NULL with n_bytes > 0.  Run it behind the per-mate trims and in front of
 * ffq_table_select_pairs.  Merging the mates by `insert`: ffq_table_pair_merge below; correcting bases inside the overlap:
 * ffq_table_pair_correct.  Not done: indels, reads above FFQ_OVERLAP_MAX_LEN bases.                                    */
typedef struct ffq_overlap_rules {
    int32_t min_overlap;     /* 1..FFQ_OVERLAP_MAX_LEN; fastp's default 30 */
    int32_t max_diff;        /* 0..FFQ_OVERLAP_MAX_LEN; fastp's default 5  */
    int32_t diff_permille;   /* 0..1000;                fastp's default 200 */
    int32_t trim;            /* 0: analyse only, rows copied unchanged; 1: cut */
} ffq_overlap_rules;
#define FFQ_OVERLAP_MAX_LEN    512
#define FFQ_OVERLAP_HIST_WORDS (2 * FFQ_OVERLAP_MAX_LEN + 1)   /* insert sizes 0..1024 */
#define FFQ_OVERLAP_COUNTS     6
int ffq_table_pair_overlap(ffq_ctx *ctx, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                           const ffq_overlap_rules *rules, int64_t *d_out1, int64_t *d_out2,
                           int32_t *d_insert, uint64_t *d_hist, int accumulate,
                           int64_t counts[FFQ_OVERLAP_COUNTS]);

/* FASTQ text from (buffer, table): what a pipeline that excluded reads by deleting rows and trimmed them by editing rows
 * ("to avoid saving a FASTQ file after each filtering or read-trimming step", doc/user-guide.rst:196-204) saves at its
 * end.  Row p renders as
 *     "@" + buf[p0 + 1 : p1] + "\n" + buf[p2 : p3] + "\n+\n" + buf[p4 : p5] + "\n"
 * -- the three slices entryfunc cuts (fastqandfurious.py:161-171), copied verbatim (a wrapped record keeps its embedded
 * newlines), and six literal bytes; the '+' line is always the bare "+", a repeated header is not copied; a row whose
 * pos2..pos5 a trim moved renders the trimmed read.  A row is RENDERABLE if all six positions - add are >= 0,
 * p0 + 1 <= p1, p2 <= p3, p4 <= p5 and every slice lies inside the buffer (it may end at its end; with sentinel,
 * coordinate 0 is the virtual "\n": never read).  Every other row -- FASTA rows (-1), rows that point outside -- renders
 * as zero bytes and is counted as skipped; no byte outside [d_buf, d_buf + n_bytes) is read.  Rows are independent: any
 * order, repeated, overlapping; the output follows table order.  d_buf / n_bytes / sentinel / add: as for
 * ffq_table_gather_column.  d_table 16-byte aligned; d_out: out_cap bytes, no alignment asked; d_off: n_rows + 1
 * offsets (d_off[i] = where row i's record starts in d_out, d_off[n_rows] = the total), or NULL.  stats = {bytes
 * rendered, rows rendered, rows skipped}.  FFQ_E_TABLE_FULL: out_cap is smaller than the total -- stats[0] holds the
 * need, d_off is written, d_out is not touched.  FFQ_E_ARG: a scan pending on the context.  One host wait.
 * A read of length 0 renders as "@h\n\n+\n\n".  A file with such records is read back record for record by the Python
 * scanner (fastqandfurious.entrypos) ONLY: the device scanners answer as the reference's C scanner does, which looks for
 * the end of a sequence behind its first byte and reads an empty record and its successor as one longer record, without
 * an error.  Filter with min_seq_len >= 1 in front of the rendering: that is what makes the text safe for the GPU
 * scanner and for other tools.                                                                                        */
int ffq_table_render_fastq(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                           const int64_t *d_table, int64_t n_rows, uint8_t *d_out, int64_t out_cap, int64_t *d_off,
                           int64_t stats[3]);

/* Unique molecular identifiers (UMIs): the first bases of a read that tag the molecule and are no part of the fragment.  They
 * are taken off the read before anything else looks at it and kept in the read's NAME, where aligners and umi_tools-style
 * deduplicators look for them: what `fastp --umi --umi_loc read1|read2|per_read --umi_len N [--umi_skip M] [--umi_prefix P]`
 * is for.  The rule below follows fastp's DOCUMENTED behaviour from memory: fastp's source was not at hand, the rule has NOT
 * been checked against it, and no parity is claimed.
 *
 * THE TAKE, ffq_table_take_umi, MODIFIES rows.  For one row, n = pos3 - pos2; len in 1..64, skip in 0..64:
 *     eligible = pos2..pos5 - add all >= 0, in order, inside the buffer, pos3 - pos2 == pos5 - pos4 (with sentinel, coordinate
 *                0 is the virtual "\n": a line with bytes in it may not begin there), no byte of the sequence and no byte of
 *                the quality is "\n", and pos2 == pos1 + 1 (a scanned, unwrapped record: the sequence begins behind the
 *                header's newline)
 *     if not eligible:   the row is copied unchanged and counted as skipped
 *     else if n < len:   the row is unchanged (and not skipped): a read shorter than its tag keeps its bases
 *     else:              cut = min(len + skip, n);  the row becomes pos0, pos1, pos2 + cut, pos3, pos4 + cut, pos5
 * A read may go to length 0.  pos0 and pos1 never move -- no pass moves them -- so the tag of a row the take changed still
 * lies at buf[pos1 + 1 : pos1 + 1 + len] when the row is rendered, whatever selects, dedups and pair compactions it went
 * through: the take needs no side table.  stats = {rows changed, bases removed, rows skipped}; d_out MAY be d_table; the other
 * arguments, FFQ_E_ARG and the one host wait are ffq_table_trim_poly's.  No byte outside the row's two checked lines is read.
 *
 * A CARRIER.  A source row carries a tag under len if pos1 - add >= 0 and pos2 - add >= 0, pos1 + 1 + len <= pos2,
 * [pos1 + 1, pos1 + 1 + len) lies inside its buffer (it begins behind coordinate 0) and none of those bytes is "\n"; the tag is
 * those bytes.  Behind the take a scanned record carries a tag exactly if the take changed it (DESIGN.md 4w says why no later
 * pass makes a carrier of a row the take left alone).
 *
 * THE INSERT, ffq_table_render_fastq_umi, renders `rows` as ffq_table_render_fastq does, with the tag in the name.  src1 is
 * the table whose row i may carry the tag of read 1 (needed for FFQ_UMI_READ1 and _PER_READ), src2 the same for read 2 (_READ2
 * and _PER_READ); either may be `rows` itself or a table over another buffer with another add and sentinel; the rows are in
 * step.  For row i, with h = buf[pos0 + 1 : pos1] of `rows`:
 *     k    = index of the first ' ' or '\t' in h, len(h) if there is none
 *     tag  = tag1 | tag2 | tag1 + "_" + tag2                          (by loc)
 *     ins  = delim + (prefix + "_" if prefix_len else "") + tag
 *     if row i is renderable and every source row the location names is a carrier:
 *         "@" + h[:k] + ins + h[k:] + "\n" + seq + "\n+\n" + qual + "\n"
 *     else: exactly what ffq_table_render_fastq renders (nothing, for a row that is not renderable)
 * stats = {bytes rendered, rows rendered, rows skipped, rows tagged}.  Renderability, d_off, FFQ_E_TABLE_FULL (stats[0] holds
 * the need, d_off is written, d_out is not touched), "any order, repeated, overlapping" and "no byte outside the buffers is
 * read" are ffq_table_render_fastq's.  FFQ_E_ARG: loc, len, skip, delim (0x21..0x7E), prefix_len (0..16) or a prefix byte
 * (A-Z a-z 0-9) out of range, a source the location needs missing, misaligned tables, a scan pending.  One host wait.
 * Not done: UMIs in the index part of a header (index1 / index2), UMI with merged pairs, separate lengths per mate.      */
#define FFQ_UMI_READ1 1
#define FFQ_UMI_READ2 2
#define FFQ_UMI_PER_READ 3
typedef struct ffq_umi_rules {
    int32_t loc;            /* FFQ_UMI_READ1 | _READ2 | _PER_READ */
    int32_t len;            /* 1..64: bases of the UMI */
    int32_t skip;           /* 0..64: bases dropped behind it */
    uint8_t delim;          /* 0x21..0x7E, default ':' */
    uint8_t prefix_len;     /* 0..16 */
    uint8_t prefix[16];     /* bytes of [A-Za-z0-9] */
} ffq_umi_rules;
int ffq_table_take_umi(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                       const int64_t *d_table, int64_t n_rows, int umi_len, int umi_skip, int64_t *d_out, int64_t stats[3]);
int ffq_table_render_fastq_umi(ffq_ctx *ctx, const ffq_table_view *rows, int64_t n_rows, const ffq_table_view *src1,
                               const ffq_table_view *src2, const ffq_umi_rules *rules, uint8_t *d_out, int64_t out_cap,
                               int64_t *d_off, int64_t stats[4]);

/* Device bytes written as BGZF (SAM specification 4.1: what bgzip writes, gzip members that say how long they are), deflated
 * on the device: what a pipeline that ends in .fq.gz does with the text ffq_table_render_fastq leaves there.
 * CONTAINER.  d_src[0, n_bytes) is cut into blocks of FFQ_BGZF_BLOCK_BYTES = 65280 bytes, the last one shorter.  Block k
 * becomes one gzip member: 18 bytes of header (1f 8b 08 04, no time, XFL 0, OS ff, XLEN 6, the subfield "BC" with BSIZE =
 * the member's bytes - 1), ONE raw deflate stream of one block with BFINAL set, CRC-32 and ISIZE.  The members stand back to
 * back in d_out; d_member_off (NULL, or members + 1 words): where each begins, and the total.  The empty member that ends a
 * BGZF FILE is not written: that is the file writer's business (ffq_bgzf_eof_block gives its 28 bytes).
 * BOUND.  The deflate block is BTYPE=2 -- literals and (length, distance) pairs under two Huffman codes built from the
 * block's own counts, at most 15 bits, the code lengths themselves under a third of at most 7 bits, without run-length
 * symbols -- unless that stream would be longer than a stored block: then the member is one stored block (BTYPE=0), data +
 * 31 bytes.  So no member exceeds 65536 bytes, and ffq_deflate_bgzf_bound(n) = n + 31 * ceil(n / 65280) holds any result.
 * MATCH RULE.  Positions are taken in rounds of FFQ_DEFLATE_ROUND_POSITIONS.  Every position of a round with four bytes
 * behind it first looks up, under a hash of those four bytes, the most recent position of an EARLIER round with that hash;
 * then the round's positions are entered.  The second candidate of a position is distance 1 (runs).  The block is cut into
 * segments of FFQ_DEFLATE_SEG_BYTES and each is parsed greedily on its own: at a position the longer candidate is taken if
 * it agrees in 4 bytes or more (a tie: distance 1), at most 258 and never across the end of the segment; else the byte is a
 * literal.  A candidate farther back than 32768 is refused.  No lazy matching.  The output is DETERMINISTIC: the same
 * bytes give the same members on every call and every device.
 * stats = {bytes in, bytes out, members, members stored}.  n_bytes == 0 is valid and writes nothing (d_member_off: one
 * zero).  FFQ_E_TABLE_FULL: out_cap is smaller than the total -- stats[1] holds the need, d_member_off is written, d_out
 * is not touched.  FFQ_E_ARG: a scan pending on the context.  Scratch is the context's and grows with n_bytes (a 64 KiB
 * slot per block, in which the member is built before its place is known).  One host wait.  d_src and d_out: no alignment
 * asked, and they must not overlap.                                                                                     */
#define FFQ_BGZF_BLOCK_BYTES 65280
#define FFQ_DEFLATE_SEG_BYTES 256
#define FFQ_DEFLATE_ROUND_POSITIONS 1024
#define FFQ_DEFLATE_GRID_BLOCKS 256           /* blocks deflated at a time: an input of more takes the device several passes */
#define FFQ_DEFLATE_COUNTS 4
int64_t ffq_deflate_bgzf_bound(int64_t n_bytes);
int ffq_deflate_bgzf(ffq_ctx *ctx, const uint8_t *d_src, int64_t n_bytes, uint8_t *d_out, int64_t out_cap,
                     int64_t *d_member_off /* NULL or members + 1 */, int64_t stats[FFQ_DEFLATE_COUNTS]);
void ffq_bgzf_eof_block(uint8_t out[28]);

/* The two mates of a pair merged into ONE read and rendered as FASTQ text (`fastp --merge`, PEAR, FLASH, NGmerge): mate 2
 * is read backwards and complemented, and inside the overlap the base and the quality come from whichever mate is surer.
 * For input pair k, with j = d_ord ? d_ord[k] : k, ins = d_insert[j], a / qa = mate 1's sequence and quality (n1 bytes),
 * b / qb = mate 2's (n2 bytes) -- all four as the rows stand NOW, behind any trim -- and o = ins - n2, the pair is MERGEABLE
 * if both rows are eligible as ffq_table_stats asks (pos2..pos5 - add inside the buffer and in order, the two lines of one
 * length, no line with bytes in it at the sentinel's coordinate 0), mate 1's header slice is renderable as
 * ffq_table_render_fastq asks (p0 >= 0, p0 + 1 <= p1, inside the buffer), n1 and n2 <= FFQ_OVERLAP_MAX_LEN, ins >= 0 and
 * -n2 < o < n1 (the overlap min(n1, n2 + o) - max(0, o) has at least one position).  Then
 *     L = o < 0 ? n2 + o : max(n1, n2 + o)
 *     for p in [0, L):
 *         inA = p < n1;  j2 = p - o;  inB = 0 <= j2 < n2;  bi = n2 - 1 - j2        (at least one of inA, inB holds)
 *         takeB = inA && inB ? qb[bi] > qa[p] : !inA        (bytes compared unsigned; on a tie mate 1 wins)
 *         base[p] = takeB ? comp(b[bi]) : a[p];   qual[p] = takeB ? qb[bi] : qa[p]
 *     comp: A<->T, C<->G, a<->t, c<->g; every other byte unchanged
 *     text = "@" + buf1[p0 + 1 : p1] + "\n" + base + "\n+\n" + qual + "\n"
 * For o < 0, a[L:] and the first -o bases of the reverse complement are adapter and are left out.  o is taken against the
 * CURRENT n2, so the text is the same whether ffq_table_pair_overlap ran with trim 1 or 0: behind the cut n2' = ins,
 * o' = 0, and bi names the same byte.  Every other pair -- ins of -1 or -2, an ins that does not fit these rows, FASTA rows,
 * rows written by hand, long reads, wrapped records whose lengths differ -- is not merged: both its rows go to the rest
 * tables unchanged, in order.  Positions and ranges are checked again here: no byte outside either buffer is read whatever
 * d_insert holds.  "\n" is not looked for inside the lines: bytes are taken as they are, as the render does.
 * THREE DIFFERENCES from fastp: the higher quality always wins and keeps its quality (fastp keeps mate 1's base unless its
 * correction rule fires); the header is mate 1's, verbatim (no merged_x_y comment); no insertions or deletions.
 * d_insert: DEVICE memory, int32 (ffq_table_pair_overlap's); d_ord (NULL: the identity): DEVICE memory, where pair k's
 * insert size is (ffq_table_select_pairs' d_idx); d_text: text_cap bytes, no alignment asked; d_off (NULL: none):
 * n_pairs + 1 offsets, a pair that is not merged has zero bytes; d_rest1 / d_rest2: room for n_pairs rows each, 16-byte
 * aligned, NOT the input tables; d_rest_ord (NULL: none): j of every pair that is not merged; *n_rest: their number.
 * counts: [0] pairs merged, [1] pairs not merged, [2] bytes of text, [3] bases of the merged reads, [4] positions inside
 * overlaps, [5] of those, positions taken from mate 2; [0] + [1] == n_pairs.  FFQ_E_TABLE_FULL: text_cap is smaller than
 * the total -- counts[2] holds the need, d_off and the rest tables are written, d_text is not touched.  FFQ_E_ARG: d_insert
 * NULL, a misaligned table or array, a scan pending on the context, d_buf NULL with n_bytes > 0.  n_pairs == 0 is valid.
 * One host wait.  Correcting the mates' bases in place, for pairs that are not merged too: ffq_table_pair_correct.      */
#define FFQ_MERGE_COUNTS 6
int ffq_table_pair_merge(ffq_ctx *ctx, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                         const int32_t *d_insert, const int64_t *d_ord, uint8_t *d_text, int64_t text_cap, int64_t *d_off,
                         int64_t *d_rest1, int64_t *d_rest2, int64_t *d_rest_ord, int64_t *n_rest,
                         int64_t counts[FFQ_MERGE_COUNTS]);

/* Mismatched bases inside the overlap of a pair's mates corrected IN THE BUFFERS (`fastp --correction`): where both mates read
 * the same position and disagree, and one call is sure while the other is poor, the poor base and its quality are replaced by
 * the sure ones.  THE RULE STATED HERE IS THE SPECIFICATION; fastqandfurious.correct_mates is its host statement.  Run it behind
 * ffq_table_pair_overlap and in front of ffq_table_select_pairs.  For pair k, with ins = d_insert[k], a / qa = mate 1's
 * sequence and quality (n1 bytes), b / qb = mate 2's (n2 bytes) -- all four as the rows stand NOW -- and o = ins - n2, the pair
 * is LOOKED AT if both rows are eligible as ffq_table_pair_merge asks of pos2..pos5 (inside the buffer and in order, the two
 * lines of one length, no line with bytes in it at the sentinel's coordinate 0; the header is not asked about), n1 and
 * n2 <= FFQ_OVERLAP_MAX_LEN, ins >= 0 and -n2 < o < n1.  Every other pair is left untouched and counted as not looked at.  Then
 *     G = qual_base + good_quality;  B = qual_base + bad_quality            (bytes; qualities are compared unsigned)
 *     for p in [max(0, o), min(n1, n2 + o)):
 *         bi = n2 - 1 - (p - o);  ca = cls(a[p]);  cb = cls(b[bi])          (cls: the classes of ffq_table_stats)
 *         if ca < 4 and cb < 4 and ca == 3 - cb: nothing                    (ffq_table_pair_overlap's MATCH)
 *         else, a MISMATCH POSITION:
 *             if   qa[p]  >= G and qb[bi] <= B and ca < 4:  b[bi] = comp(a[p]);  qb[bi] = qa[p]      (mate 2 corrected)
 *             elif qb[bi] >= G and qa[p]  <= B and cb < 4:  a[p]  = comp(b[bi]); qa[p]  = qb[bi]     (mate 1 corrected)
 *     comp: ffq_table_pair_merge's (A<->T, C<->G, the case kept)
 * An N is never written over a base; an N with a poor quality IS replaced by a sure base.  o is taken against the CURRENT n2, so
 * the result is the same whether ffq_table_pair_overlap ran with trim 1 or 0 (behind the cut n2' = ins, o' = 0, and bi names the
 * same byte: ffq_table_pair_merge's argument).  fastp's gate "more than 5 differences: skip the pair" needs no word here: a
 * pair has an insert size only if its mismatches are <= max_diff.  "\n" is not looked for: bytes are taken as they are, as in
 * the merge.  The pass is IDEMPOTENT (a corrected position matches: a second run changes nothing and corrects 0), and the
 * positions of a pair are independent of each other.  TWO DIFFERENCES from fastp: matching is by class, so N never matches
 * (fastp compares bytes); fastp's per-read "corrected" flags are not kept.
 * CONTRACT.  Only the bytes named above are written -- one byte at a time, never a block around them.  No byte outside either
 * [d_buf, d_buf + n_bytes), and none outside the two rows' checked sequence and quality ranges, is read or written, whatever
 * d_insert holds.  UNLIKE EVERY OTHER TABLE CALL, THE ROWS OF DIFFERENT PAIRS MUST NOT SHARE BYTES: pairs are corrected
 * concurrently, and a byte two rows name would be read by one pair while the other rewrites it.  (The rows of a scanned fill
 * never do.)  m1->d_buf / m2->d_buf are WRITTEN through, although the view declares them const: they must be device memory the
 * caller may modify.
 * counts: [0] pairs looked at, [1] pairs with at least one correction, [2] bases corrected in mate 1, [3] in mate 2, [4]
 * mismatch positions met, [5] pairs not looked at; [0] + [5] == n_pairs.  matrix (NULL: not wanted):
 * matrix[4 * (class before, 0..4) + (class after, 0..3)] = corrections of that kind, both mates together.  n_pairs == 0 is
 * valid.  One host wait.  FFQ_E_ARG: rules NULL or out of range (0 <= bad_quality < good_quality, qual_base 0..255,
 * qual_base + good_quality <= 255), d_insert NULL or misaligned, a misaligned table, a scan pending on the context, d_buf NULL
 * with n_bytes > 0.  Not done: indels, reads above FFQ_OVERLAP_MAX_LEN bases.                                            */
typedef struct ffq_correct_rules {
    int32_t good_quality;    /* a call at or above it is sure; fastp's 30 */
    int32_t bad_quality;     /* a call at or below it is poor; fastp's 14 */
    int32_t qual_base;       /* 33 or 64 */
} ffq_correct_rules;
#define FFQ_CORRECT_COUNTS 6
#define FFQ_CORRECT_MATRIX_WORDS 20
int ffq_table_pair_correct(ffq_ctx *ctx, const ffq_table_view *m1, const ffq_table_view *m2, int64_t n_pairs,
                           const int32_t *d_insert, const ffq_correct_rules *rules, int64_t counts[FFQ_CORRECT_COUNTS],
                           int64_t matrix[FFQ_CORRECT_MATRIX_WORDS]);

/* ---- duplicate reads and pairs: sequence keys, the first copy wins (`fastp --dedup`, clumpify, czid-dedup) ---------------
 * There is no reference implementation of this: THE RULE STATED HERE IS THE SPECIFICATION.  fastqandfurious.seq_key and
 * pair_key are its host statement in Python, ffq_seq_key_host / ffq_pair_key_host the same in C.
 *
 * KEY OF A ROW.  seq = buf[pos2 : pos3] as the row stands when the pass runs, n = len(seq).  With sm the splitmix64 finaliser
 *     sm(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31
 *     w_k  = the 4 bytes seq[4k .. 4k + 4) as a little-endian uint32, bytes behind the end taken as 0, k = 0 .. ceil(n / 4) - 1
 *     S    = sum over k of sm( ((k + 1) << 32) | w_k )          (mod 2^64)
 *     key  = sm( S + n * 0x9e3779b97f4a7c15 );   a key of 0 becomes 1
 * Words are counted from the sequence's first byte, wherever that lies in memory.  The sum is commutative on purpose: the
 * lanes and steps of a kernel add their terms in any order and the result is bit-identical.  Bytes are taken verbatim: case
 * is not folded, 'N' is a byte like any other.  A row is KEYED if it is eligible as ffq_table_trim_adapter asks: positions
 * - add >= 0 and in order inside the buffer, pos3 - pos2 == pos5 - pos4, the sentinel's coordinate 0 never read, no "\n"
 * in the sequence.  Every other row -- wrapped records, FASTA rows (-1), rows written by hand that point outside -- gets
 * FFQ_KEY_NONE.  A read of length 0 is keyed; all empty reads share one key.  No byte outside [d_buf, d_buf + n_bytes) and
 * none outside the row's checked sequence range is read; the quality line is never read.
 * ffq_table_seq_keys: d_keys[i] = the key of row i (DEVICE memory, n_rows words, 8-byte aligned; d_table 16-byte aligned;
 * d_buf / n_bytes / sentinel / add as for ffq_table_gather_column); counts = {rows keyed, rows not keyed}.  n_rows == 0 is
 * valid.  FFQ_E_ARG: a misaligned table, a scan pending on the context.  One host wait.
 * PAIR KEY.  pk = sm( sm(k1) + k2 ), 0 becomes 1; FFQ_KEY_NONE if either mate's key is FFQ_KEY_NONE.  Ordered: (k1, k2),
 * (k2, k1) and (k1, k1) are three pairs.
 *
 * THE SET.  ffq_dedup is a device-resident set of {key, first} entries that lives across calls and grows with the file.  Every
 * row submitted gets a global ordinal g = rows submitted to this set before this call + i.  A keyed row is KEPT if and only
 * if no row with the same key and a smaller g was ever submitted, in this call or an earlier one: the first copy in file
 * order wins, whatever the scheduling.  A row with FFQ_KEY_NONE is always kept and never entered.
 * Two DIFFERENT sequences with equal 64-bit keys count as duplicates: among n reads the chance of one such false pair is
 * about n^2 / 2^65 (the birthday bound: 3e-3 for a billion reads).
 * DIFFERENCES from fastp --dedup: the set is exact on the key, not a fixed-size filter with an accuracy level; the key covers
 * the whole read as scanned, not a prefix; only reads that survive the filters compete (the stream's order, below).
 * ffq_dedup_create: expected_keys (0: the minimum table of 1024 slots) sizes the table so that this many keys enter without
 * growth; max_bytes (0: no cap) caps the table's bytes -- a table that would have to grow beyond it makes the call return
 * FFQ_E_NOMEM, with the need in ffq_last_error, BEFORE anything is launched, and the set stays as it was and usable.  The table
 * is open addressing over 16-byte slots, grown by the host to the next power of two with slots >= 2 (keys + rows of the
 * call) before a call that could fill it beyond 1/2; the old and the new table are alive together while one is rehashed
 * into the other.
 * ffq_dedup_select: row i of the call uses d_keys*[j], j = d_ord ? d_ord[i] : i, and d_idx[k] = j of kept row k: behind a
 * select whose d_idx is handed in as d_ord, what comes out still names ordinals among the scanned rows.  d_keys2 (NULL:
 * single reads): the second mates' keys -- the rows then go by their pair keys.  d_table1 / d_table2 (NULL: no rows are
 * copied; d_table2 needs d_keys2): n rows each whose kept ones go to d_out1 / d_out2, in order -- room for n rows, 16-byte
 * aligned, NOT the input tables; d_idx may be NULL; *n_out = rows kept.  drop == 0: count only -- every row is kept and
 * copied, *n_out = n, the set and the counts advance exactly as with drop != 0, so counts[1] is what would have been dropped.
 * counts: [0] rows kept, [1] duplicates, [2] rows without a key (also in [0]), [3] distinct keys in the set after the call,
 * [4] slots, [5] rehashes so far; [0] + [1] == n.  n == 0 is valid.  One host wait.  FFQ_E_ARG: misalignment, a NULL set, a
 * scan pending on the context, d_table2 without d_keys2.  FFQ_E_INTERNAL: a probe visited every slot -- no kernel of the set
 * loops without a bound.  All DEVICE memory; calls on a set follow one another (its context's stream).
 * Not done: a histogram of duplication levels, keys for wrapped records, reverse-complement-aware keys, a set larger than
 * device memory.                                                                                                        */
#define FFQ_KEY_NONE 0
int ffq_table_seq_keys(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel, int64_t add,
                       const int64_t *d_table, int64_t n_rows, uint64_t *d_keys,
                       int64_t counts[2] /* keyed, not keyed */);
uint64_t ffq_seq_key_host(const uint8_t *seq, int64_t n);          /* the rule on the host, for bindings and tests */
uint64_t ffq_pair_key_host(uint64_t k1, uint64_t k2);

typedef struct ffq_dedup ffq_dedup;
int  ffq_dedup_create(ffq_ctx *ctx, int64_t expected_keys /* 0: the minimum */, int64_t max_bytes /* 0: no cap */, ffq_dedup **out);
void ffq_dedup_destroy(ffq_dedup *d);
#define FFQ_DEDUP_COUNTS 6
int  ffq_dedup_select(ffq_dedup *d, const uint64_t *d_keys1, const uint64_t *d_keys2 /* NULL: single reads */,
                      const int64_t *d_ord /* NULL: identity */, int64_t n,
                      const int64_t *d_table1, const int64_t *d_table2,
                      int64_t *d_out1, int64_t *d_out2, int64_t *d_idx, int64_t *n_out,
                      int drop /* 0: count only, every row is kept and copied */, int64_t counts[FFQ_DEDUP_COUNTS]);

/* ---- FASTA (reference: the plug-in scanner entrypos_fasta, fastqandfurious.py:103-143) -------
 * Every COMPLETE entry of a buffer, i.e. the repeated scanner call with offset := pos[3]:
 * rows = pos0 ('>'), pos1 (header end), pos2, pos3 (the "\n" of the next "\n>") + add, -1, -1.
 * res->n_records = COMPLETE entries; res->last_status / last_pos = the last call (the entry
 * the end of the buffer cuts short: MISSING_SEQ_END with pos3 = end of the buffer, or an
 * earlier MISSING_* code; MISSING_SEQHEADER_BEGIN if there was no entry at all);
 * res->end_offset = the offset of that last call.  sentinel: a virtual "\n" in front.  d_buf and
 * d_table must be 16-byte aligned.  FFQ_E_TABLE_FULL (res->n_records = the rows needed): rows
 * [0, table_cap - 1) are complete; pos3 of row table_cap - 1 may be -1 (its end is the next row's start). */
int ffq_scan_fasta_device(ffq_ctx *ctx, const uint8_t *d_buf, int64_t n_bytes, int sentinel,
                          int64_t offset, int64_t add, int64_t *d_table, int64_t table_cap,
                          ffq_scan_result *res);
int ffq_scan_fasta_host(ffq_ctx *ctx, const uint8_t *h_buf, int64_t n_bytes, int sentinel,
                        int64_t offset, int64_t add, int64_t *h_table, int64_t table_cap,
                        ffq_scan_result *res);

/* ---- stream front end (reference: read(), fastqandfurious.py:30-36, and the refill loop of
 * readfastq_iter, :241-279, natively over a file descriptor) ---------------------------------
 * A three-stage pipeline: chunks of fbufsize bytes are read into pinned memory by a pool of
 * helper threads, copied to the device on a copy stream, and scanned; the read of chunk k+2, the
 * copy of chunk k+1 and the scan + row copy of fill k overlap.  ffq_stream_next returns the rows
 * of ONE fill: absolute stream offsets (what entryfunc_abspos yields, :186-195), in pinned memory
 * owned by the stream and valid until the next call, together with the fill's bytes
 * (h_bytes[i] is stream offset bytes_offset + i).  end_state: FFQ_END_REFILL while more
 * follows, FFQ_END_OK with the last fill, FFQ_END_ERR_* (+ err_offset, the byte the reference's
 * ValueError names) when the stream is malformed.  A call that fails leaves the stream failed
 * (every later call fails too).  The descriptor is not closed and, when it can seek, not moved
 * either (pread).                                                                                */
typedef struct ffq_stream ffq_stream;
int  ffq_stream_open(ffq_ctx *ctx, int fd, int64_t fbufsize, ffq_stream **out);
int  ffq_stream_next(ffq_stream *s, const int64_t **h_rows, int64_t *n_rows, int *end_state,
                     int64_t *err_offset, const uint8_t **h_bytes, int64_t *n_bytes,
                     int64_t *bytes_offset);
void ffq_stream_close(ffq_stream *s);
/* The same with options.  flags = FFQ_F_DECODE_QUAL: every fill's qualities are decoded on the
 * device (array('b').frombytes(buf[pos4:pos5]); arrayadd_b(q, qual_add), doc/user-guide.rst:130-141)
 * and ffq_stream_quals hands back the int8 bytes and their offsets (n_rows + 1 entries) of
 * the fill ffq_stream_next has just returned; pinned memory, valid until the next call: record i's
 * bytes are h_qual[h_qoff[i] : h_qoff[i] + pos5(i) - pos4(i)], h_qoff[n_rows] = *n_qual_bytes = where
 * the last record's end.  Packed back to back -- or, flags = FFQ_F_DECODE_QUAL | FFQ_F_SINGLE_PASS,
 * segmented (see FFQ_F_SINGLE_PASS above) whenever the single pass takes the fill (plain four-line
 * records: the fill is read once); ffq_stream_path = ffq_scan_result.path of the last fill (6 then).
 * start: byte of the file the stream begins at (< 0: the descriptor's current position); stream
 * offsets count from there.  ffq_stream_tell: the file position behind the last chunk HANDED OUT by
 * ffq_stream_next (the reader itself runs ahead of that): where a caller that shares the file object
 * should leave it, as the reference's loop does.  A descriptor that cannot seek (a pipe) is read
 * behind poll(): closing the stream never waits for a writer that keeps the pipe open and idle, and a
 * chunk is handed over short -- which is not the end of the stream -- when nothing more has arrived
 * for 50 ms.  A chunk comes in over the link in two halves on two copy streams (two copy engines);
 * a stream that decodes -- half as many bytes go back as come in -- uses one, the engines are
 * shared between the directions (FFQ_STREAM_ONE_COPY_STREAM = 0 / 1 forces either; FFQ_STREAM_PROF=1
 * prints where a stream's time went when it closes).                                               */
int  ffq_stream_open2(ffq_ctx *ctx, int fd, int64_t fbufsize, uint32_t flags, int qual_add, int64_t start,
                      ffq_stream **out);
int  ffq_stream_quals(ffq_stream *s, const int8_t **h_qual, const int64_t **h_qoff, int64_t *n_qual_bytes);
int64_t ffq_stream_tell(ffq_stream *s);
int  ffq_stream_path(ffq_stream *s);
/* Push-down into the stream -- the reference's user guide (doc/user-guide.rst:153-180): an entryfunc that looks at the
 * read's length and builds ONE component of the entries it keeps, `buf[posarray[2]:posarray[3]] if posarray[3] -
 * posarray[2] < LENGTH_THRESHOLD else None`, so that a dropped record costs (nearly) nothing.  ffq_stream_set_filter
 * (any kind of stream, before the first ffq_stream_next; not with FFQ_F_DECODE_QUAL): every fill's table is filtered on
 * the DEVICE before anything is copied back -- ffq_stream_next then returns the rows with min_seq_len <= pos3 - pos2 <=
 * max_seq_len only, in order -- and, column != FFQ_COL_NONE, that component of every kept row is gathered there into a
 * packed stream (header as entryfunc cuts it, fastqandfurious.py:161-171: buf[pos0 + 1 : pos1]; + value_add per byte:
 * -33 on the quality is the Phred decode of the kept records only).  ffq_stream_selected, for the fill just returned:
 * h_index[i] = the ordinal of kept row i among the n_scanned records of the fill (a caller that owes one item per
 * record -- the guide's loop sees None for a dropped one -- puts the kept ones back by it); bytes of kept row i =
 * h_col[h_coloff[i] : h_coloff[i + 1]].  Pinned memory of the stream, valid until the next call.                     */
#define FFQ_COL_NONE     0
#define FFQ_COL_HEADER   1
#define FFQ_COL_SEQUENCE 2
#define FFQ_COL_QUALITY  3
int  ffq_stream_set_filter(ffq_stream *s, int64_t min_seq_len, int64_t max_seq_len, int column, int value_add);
int  ffq_stream_selected(ffq_stream *s, const int64_t **h_index, int64_t *n_scanned, const int8_t **h_col,
                         const int64_t **h_coloff, int64_t *n_col_bytes);
/* Quality trimming in the stream (any kind of stream, before the first ffq_stream_next; not with FFQ_F_DECODE_QUAL,
 * whose qualities are decoded beside the scan: a filtered stream gathers the TRIMMED quality, column = FFQ_COL_QUALITY,
 * value_add): every fill's table is trimmed in place on the device (ffq_table_trim_quality) right behind the scan -- in
 * front of the filter, the column gather and the rows' copy back, which all see the trimmed rows; pos0 / pos1 and the
 * refill (it goes by the scan's end offset) are untouched.  ffq_stream_trimmed: {rows changed, bases removed, rows
 * skipped} of the fill ffq_stream_next has just returned.                                                          */
int  ffq_stream_set_trim(ffq_stream *s, int qual_base, int cutoff_front, int cutoff_back);
int  ffq_stream_trimmed(ffq_stream *s, int64_t stats[3]);
/* 3' adapter trimming in the stream (the rules of ffq_stream_set_trim: before the first ffq_stream_next, not with
 * FFQ_F_DECODE_QUAL): every fill's table is adapter-trimmed in place on the device (ffq_table_trim_adapter) right BEHIND
 * the quality trim, if the stream has one -- cutadapt's own order, -q first and -a on the row as that trim left it -- and
 * in front of the filter, the column gather, the render and the rows' copy back; the refill goes by the scan's end offset.
 * `adapter` (host memory) is copied.  ffq_stream_adapter_trimmed: {rows changed, bases removed, rows skipped} of the fill
 * ffq_stream_next has just returned.                                                                                  */
int  ffq_stream_set_adapter(ffq_stream *s, const uint8_t *adapter, int adapter_len, int err_permille, int min_overlap);
int  ffq_stream_adapter_trimmed(ffq_stream *s, int64_t stats[3]);
/* Poly-tail trimming in the stream (the rules of ffq_stream_set_trim: before the first ffq_stream_next, not with
 * FFQ_F_DECODE_QUAL): every fill's table goes through ffq_table_trim_poly in place on the device -- poly-G (base 2,
 * poly_g_min_len; 0: off) BEHIND the quality trim and IN FRONT of the adapter trim, so that the adapter match is not spoiled
 * by the G tail behind the adapter; poly-X (FFQ_POLY_ANY, poly_x_min_len; 0: off) BEHIND the adapter trim.  Both are per
 * mate and in front of a pair's overlap analysis; fastp runs its poly-X behind its overlap trim: a departure.  At least one
 * of the two is on; a min_len that is on is 2..65535.  ffq_stream_poly_trimmed: {rows changed, bases removed, rows skipped}
 * of either step for the fill ffq_stream_next has just returned (zeros for a step that is off).                        */
int  ffq_stream_set_poly(ffq_stream *s, int poly_g_min_len, int poly_x_min_len);
int  ffq_stream_poly_trimmed(ffq_stream *s, int64_t stats_g[3], int64_t stats_x[3]);
/* UMIs in the stream (the rules of ffq_stream_set_trim: before the first ffq_stream_next, not with FFQ_F_DECODE_QUAL): every
 * fill's table goes through ffq_table_take_umi in place on the device BEHIND the dedup keys and the statistics IN -- they see
 * the read as read, so two reads with the same sequence and different UMIs are no duplicates -- and IN FRONT of the ends and
 * every other trim, which see the read without its UMI, as the statistics OUT do; a stream that renders puts the tag into the
 * names (ffq_table_render_fastq_umi, the rendered rows their own source), also behind ffq_stream_set_compress.  On a single
 * stream only FFQ_UMI_READ1 is valid (FFQ_E_ARG); a pair: ffq_pair_set_umi.  ffq_stream_umi_counts: {rows taken, bases
 * removed, rows skipped, rows tagged in the output} for the fill ffq_stream_next has just returned.  Not done: push-down
 * through the iterators (the rows handed out have their UMI taken, the entries built from them do not name it).          */
int  ffq_stream_set_umi(ffq_stream *s, const ffq_umi_rules *rules);
int  ffq_stream_umi_counts(ffq_stream *s, int64_t counts[4]);
/* Fixed trims and sliding-window cutting in the stream (the rules of ffq_stream_set_trim: before the first
 * ffq_stream_next, not with FFQ_F_DECODE_QUAL): every fill's table goes through ffq_table_trim_ends in place on the device
 * BEHIND the statistics IN and IN FRONT of the quality trim and every other trim -- fastp's order --, per mate and in front
 * of a pair's overlap analysis.  `rules` is copied.  ffq_stream_ends_trimmed: {rows changed, bases removed, rows skipped} of
 * the fill ffq_stream_next has just returned.                                                                          */
int  ffq_stream_set_ends(ffq_stream *s, const ffq_ends_rules *rules);
int  ffq_stream_ends_trimmed(ffq_stream *s, int64_t stats[3]);
/* Content rules in the stream (the rules of ffq_stream_set_trim: before the first ffq_stream_next, not with
 * FFQ_F_DECODE_QUAL): the select of every fill judges the rows by ffq_table_select_reads -- as the trims left them, which
 * is cutadapt's order -- and everything behind it (statistics OUT, the render, the column gather, ffq_stream_selected) sees
 * the kept rows.  A stream without a filter gets one with unbounded length and no column; ffq_stream_set_filter and this
 * call may come in either order, each keeps what the other one set.  `rules` is copied.  ffq_stream_filter_counts: the
 * eight counts of the fill ffq_stream_next has just returned, on any filtered stream (without content rules only [0] and
 * [1] are non-zero).                                                                                                  */
int  ffq_stream_set_content(ffq_stream *s, const ffq_content_rules *rules);
int  ffq_stream_filter_counts(ffq_stream *s, int64_t counts[FFQ_FILTER_COUNTS]);
/* Statistics in the stream (any kind of stream, also with FFQ_F_DECODE_QUAL, a filter, a gathered column and a render;
 * before the first ffq_stream_next): every fill's table is counted on the device (ffq_table_stats) into a block the stream
 * owns, summed over all fills.  FFQ_STATS_IN: the rows as scanned, before any trim; FFQ_STATS_OUT: the rows as handed out,
 * behind trim, adapter and filter (what is rendered and copied back).  `which` = one of them or both; both share qual_base
 * and max_cycles.  The counting adds no host wait to a fill.  ffq_stream_stats (`which`: exactly one): the totals over every
 * fill up to and including the one ffq_stream_next has just returned, copied to h_out (host memory, cap_words >=
 * FFQ_STATS_WORDS(max_cycles) words) with one wait; after any fill and after the last one.  FFQ_E_ARG: a `which` that was
 * not set, cap_words too small, set_stats behind the first fill.                                                       */
#define FFQ_STATS_IN  1   /* rows as scanned, before any trim                       */
#define FFQ_STATS_OUT 2   /* rows as handed out: behind trim, adapter and filter    */
int  ffq_stream_set_stats(ffq_stream *s, int which /* IN | OUT */, int qual_base, int max_cycles);
int  ffq_stream_stats(ffq_stream *s, int which /* exactly one */, uint64_t *h_out, int64_t cap_words);
/* FASTQ text in the stream (any kind of stream, before the first ffq_stream_next, behind ffq_stream_set_trim /
 * ffq_stream_set_filter if those are set; FFQ_E_ARG with FFQ_F_DECODE_QUAL and with a filter that gathers a column):
 * the rows of every fill -- trimmed and filtered first, if the stream does that -- are rendered on the device
 * (ffq_table_render_fastq) and the text copied back to pinned memory of the stream.  ffq_stream_rendered: the text of
 * the fill ffq_stream_next has just returned and {bytes rendered, rows rendered, rows skipped}; valid until the next
 * call.  A last record whose quality line no newline ends (the scan takes it when a byte follows its quality; a file
 * that ends with the quality's last byte is FFQ_END_ERR_FINAL_QUAL) renders with one.                               */
int  ffq_stream_set_render(ffq_stream *s);
int  ffq_stream_rendered(ffq_stream *s, const uint8_t **h_fastq, int64_t *n_fastq_bytes, int64_t stats[3]);
/* The text compressed in the stream (before the first ffq_stream_next; FFQ_E_ARG unless the stream renders): with
 * FFQ_COMPRESS_BGZF every fill's text is written as BGZF members on the device, behind the render (ffq_deflate_bgzf over at
 * most fill + 1 bytes), and ONLY THE MEMBERS are copied back.  ffq_stream_compressed: the members of the fill
 * ffq_stream_next has just returned -- whole members, so the fills' members written one behind another, and
 * ffq_bgzf_eof_block once at the end, are a BGZF file -- and {bytes in, bytes out, members, members stored}; pinned memory,
 * valid until the next call.  ffq_stream_rendered then keeps its three counts and returns *h_fastq = NULL: the text never
 * leaves the device.  A stream without this setter does exactly what it did.                                          */
#define FFQ_COMPRESS_NONE 0
#define FFQ_COMPRESS_BGZF 1
int  ffq_stream_set_compress(ffq_stream *s, int mode);
int  ffq_stream_compressed(ffq_stream *s, const uint8_t **h_bgzf, int64_t *n_bytes, int64_t stats[FFQ_DEFLATE_COUNTS]);
/* Duplicate removal in the stream (the rules of ffq_stream_set_trim: before the first ffq_stream_next, FFQ_E_ARG with
 * FFQ_F_DECODE_QUAL).  The stream owns one ffq_dedup (expected_keys, max_bytes: ffq_dedup_create's) for its whole life.  The
 * keys of every fill's rows are taken in FRONT of the trims, on the rows as scanned (ffq_table_seq_keys) -- two PCR copies
 * whose quality trims ended at different bases are still one read, and a table does not remember a row's end once a trim
 * has moved it --, and the set is asked right BEHIND the select (ffq_dedup_select with the select's ordinals), so that a
 * read never loses to a copy the filters dropped.  Everything behind sees the rows that remain: statistics OUT, render,
 * column gather, rows back, ffq_stream_selected (whose ordinals still name the scanned records).  drop == 0: counted only,
 * every row stays.  A stream with dedup counts as filtered (unbounded, ruleless), as ffq_stream_set_content arranges it.  A
 * fill without records launches nothing.  ffq_stream_dedup_counts: the six counts over EVERY fill up to the one
 * ffq_stream_next has just returned -- [0] to [2] summed over the fills, [3] to [5] the set as it stands.              */
int  ffq_stream_set_dedup(ffq_stream *s, int drop, int64_t expected_keys, int64_t max_bytes);
int  ffq_stream_dedup_counts(ffq_stream *s, int64_t counts[FFQ_DEDUP_COUNTS]);
/* The same over a gzip-compressed file (what FORMAT_OPENERS['gz'] / automagic_open hand to
 * readfastq_iter, fastqandfurious.py:282-334): the stream's reader thread inflates (zlib; concatenated
 * members, zero padding behind the last one) straight into the pinned chunk buffers -- decompression
 * is the feeder stage of the pipeline, fbufsize counts DECOMPRESSED bytes, stream offsets are offsets
 * of the decompressed stream.  start: byte of the compressed file the first member begins at.      */
int  ffq_stream_open_gzip(ffq_ctx *ctx, int fd, int64_t fbufsize, uint32_t flags, int qual_add, int64_t start,
                          ffq_stream **out);
/* Members that say how long they are -- the BGZF blocks bgzip writes ("BC" extra field, SAM specification
 * section 4.1) -- are located without inflating anything and inflated side by side by FFQ_GZ_THREADS threads
 * (default: the host's cores, at most 32; 1 = one member at a time), each straight into its place in the
 * chunk, by this build's own decoder (csrc/ffq_pgz.h; zlib for a member it does not take); every member is checked
 * against the length and CRC-32 of its trailer, and a file that is not what
 * its headers promise goes through the one-at-a-time inflate from that member on (same bytes or same error).
 *
 * ffq_gunzip_fd: that reader on its own, no device involved -- the file behind fd (from its current
 * position; a pipe works) inflated into h_dst in calls of `chunk` bytes as the stream's reader thread makes
 * them.  threads <= 0: the default.  Returns the number of bytes written, FFQ_E_TABLE_FULL if the file holds
 * more than cap, FFQ_E_ARG for corrupt input (ffq_last_error says what); *n_parallel_members (optional):
 * how many members were inflated side by side.                                                         */
int64_t ffq_gunzip_fd(int fd, uint8_t *h_dst, int64_t cap, int64_t chunk, int threads, int64_t *n_parallel_members);
/* A member that does NOT say how long it is -- what plain `gzip` writes: one deflate stream -- is inflated by
 * the same threads when the file is a regular one (csrc/ffq_pgz.h): the compressed bytes are cut into chunks
 * (FFQ_PGZ_CHUNK, default 1 MiB; two per thread and batch), every chunk but the first of a batch enters the
 * stream at the first bit that parses as a dynamic-Huffman block header and inflates into 16-bit symbols
 * (a literal, or a reference into the 32 KiB it was not given), a chunk ends at the first accepted block
 * boundary behind its range, the stitch step takes a chunk if it starts at the bit its predecessor ended at,
 * and the symbols become bytes -- and a CRC-32, checked against the member's trailer -- side by side.  zlib
 * keeps the last word: whatever the engine does not take (a decode error, a block longer than a batch, the
 * end of the file inside a block) makes it stop at the last block boundary it committed, and the serial
 * inflate goes on from that bit (same bytes or the same error).  Members of less than FFQ_PGZ_MIN (4 MiB)
 * compressed bytes, pipes and FFQ_GZ_THREADS=1 go through zlib alone.
 * ffq_gunzip_stats: process-wide counters of that engine since the library was loaded --
 * out[0] batches, [1] chunks taken, [2] chunks not taken, [3] times it gave up, [4] members finished.    */
void ffq_gunzip_stats(int64_t out[5]);
/* A byte RANGE of a BGZF file (bgzip's format: gzip members of at most 64 KiB of data that say how long they are) on its
 * own, host only: the members whose FIRST byte lies in [c_lo, c_hi) of the compressed file -- the first one found by
 * its signature and proven by the chain of headers behind it, nothing inflated to find it -- inflated side by side
 * (threads; 0 = as ffq_gunzip_fd) into h_dst.  h_dst = NULL, cap = 0: nothing is inflated, *n_out = the bytes the
 * members' trailers promise (the pass that sizes the buffer and, summed over the ranks that share a file, gives the cut
 * points of the uncompressed stream).  *c_first / *c_end: file offsets of the first member taken and behind the last
 * (rank r's c_end is rank r + 1's c_first when their shares meet).  FFQ_E_ARG with "gzip: " in the text: not BGZF, cut
 * short, or a member that does not inflate to its trailer's length and CRC-32; FFQ_E_TABLE_FULL: more than cap bytes.
 * What it stands for: the reference's loop over gzip.open(...) (fastqandfurious.py:241-279), per rank of a file that
 * several GPUs read together (sharded.BgzfFileShard).                                                              */
int  ffq_bgzf_range(int fd, int64_t c_lo, int64_t c_hi, uint8_t *h_dst, int64_t cap, int threads,
                    int64_t *c_first, int64_t *c_end, int64_t *n_out, int64_t *n_members);
/* The same without a reader thread, for sources only the host can read (any object with a read() /
 * readinto(): BytesIO, bz2, lzma, sockets ...): the host asks where the next chunk goes
 * (ffq_stream_push_buffer: pinned memory, *cap = fbufsize bytes of room), writes up to *cap bytes
 * there itself and says how many it wrote and whether the source is exhausted (ffq_stream_push: the
 * reference's read(), fastqandfurious.py:30-36, with eof decided by the caller); ffq_stream_next then
 * scans that fill.  Up to two chunks may be pushed ahead of the one being consumed.               */
int  ffq_stream_open_push(ffq_ctx *ctx, int64_t fbufsize, uint32_t flags, int qual_add, ffq_stream **out);
int  ffq_stream_push_buffer(ffq_stream *s, uint8_t **dst, int64_t *cap);
int  ffq_stream_push(ffq_stream *s, int64_t n, int eof);

/* ---- paired-end files: two streams whose i-th records are mates (R1.fq.gz / R2.fq.gz) ---------------------------------
 * ffq_pair walks two ffq_streams in lockstep so that mates are trimmed, judged and kept or dropped TOGETHER and the two
 * outputs stay record for record in step.  Both streams are configured beforehand with the setters above -- set_trim,
 * set_adapter (its own adapter per mate: cutadapt -a / -A), set_filter without a column, set_content, set_stats,
 * set_render --; they must be fresh (no fill handed out), on the same context and opened without FFQ_F_DECODE_QUAL.  A
 * stream without a filter counts as unbounded and ruleless; both without one: every pair is kept.  After ffq_pair_open,
 * ffq_stream_next on either stream is FFQ_E_ARG: the pair walks them.
 *
 * The fills of two streams never hold the same number of records.  Each mate keeps its current fill and a window of its
 * rows that are not yet paired.  A ROUND (ffq_pair_next) first advances every mate whose window is empty and whose stream
 * has not ended -- the stream's own wait, take and scan, with carry and refill exactly as ffq_stream_next does them --,
 * takes m = min(rows left in 1, rows left in 2) and runs ONE table chain over those m rows of both fills: the names check
 * (ffq_table_pair_names, check_names != 0), statistics IN, quality trim, adapter trim, the mates' overlap
 * (ffq_table_pair_overlap, if ffq_pair_set_overlap asked for it: both slices edited in place), ffq_table_select_pairs under
 * pair_filter, statistics OUT, render, copies back; then both windows move by m.  A mate's fill stays resident until its
 * window is empty, so no row is processed or counted twice.  *n_pairs_in = m, *n_pairs_out = pairs kept; m may be 0 (a
 * fill without a complete record; the round that finds the end).  After each round the per-stream accessors report that
 * mate's share of it: ffq_stream_rendered, _trimmed, _adapter_trimmed, _stats and _filter_counts (that mate's hist of
 * ffq_table_select_pairs).  ffq_pair_rows: the kept rows of a mate (n_pairs_out of them) and the fill they point into;
 * ffq_pair_selected: h_index[k] = the ordinal, among the round's m pairs, of kept pair k, and the five pair counts.
 * Pinned memory, valid until the next ffq_pair_next.
 * ffq_pair_wants: bit 0 / bit 1 set: that mate takes a new chunk at the next ffq_pair_next -- a push stream must have one
 * pushed first.
 * *end_state: FFQ_END_REFILL while more follows; FFQ_END_OK with the round after which both mates are ended and empty; a
 * mate's own FFQ_END_ERR_* in the round in which that mate's rows run out (*err_mate = 1 or 2, *err_offset the stream's:
 * where ffq_stream_next reports it; mate 1 before mate 2);
 *     FFQ_END_ERR_PAIR_COUNT  one mate is ended and empty while the other still holds a record: *err_mate is the longer
 *                             one, *err_offset pos0 of its first unpaired record;
 *     FFQ_END_ERR_PAIR_NAMES  the names check found a different pair: *err_offset is the global ordinal of that pair; the
 *                             round hands out nothing, earlier rounds stand (h_rows of ffq_pair_rows then holds ONE row, that
 *                             mate's record of the different pair, for the caller's message).
 * After any state but FFQ_END_REFILL the pair is done.  ffq_pair_close does not close the two streams.
 * ffq_pair_set_overlap: every round analyses, and with rules->trim cuts by, the overlap of the mates behind the per-mate
 * trims and in front of the filter; before the first ffq_pair_next only (FFQ_E_ARG afterwards, and for a field out of
 * range); NULL switches it off, and ffq_pair_set_merge's merging with it.  ffq_pair_overlap: counts = the six counts of the last round; h_hist (HOST memory, NULL: not
 * wanted; cap_words >= FFQ_OVERLAP_HIST_WORDS): the insert sizes of every round so far, as ffq_stream_stats reports its
 * totals; one host wait.  FFQ_E_ARG without ffq_pair_set_overlap.
 * ffq_pair_set_merge (on != 0; before the first ffq_pair_next only; FFQ_E_ARG without ffq_pair_set_overlap): behind
 * ffq_table_select_pairs every round merges the kept pairs the rule of ffq_table_pair_merge can merge, with the insert sizes
 * the round's overlap pass found.  Those pairs leave the two ordinary outputs: what ffq_pair_rows, ffq_pair_selected's
 * h_index, the per-mate renders and statistics OUT hand out are then the kept pairs that were NOT merged, *n_pairs_out their
 * number; pairs[0] of ffq_pair_selected still counts every pair the filter kept.  ffq_pair_merged: the round's merged text
 * (pinned memory, valid until the next ffq_pair_next; *n_bytes == counts[2]) and the six counts of ffq_table_pair_merge;
 * counts may be NULL.  FFQ_E_ARG without ffq_pair_set_merge.
 * ffq_pair_set_compress (FFQ_COMPRESS_BGZF; before the first ffq_pair_next only; FFQ_E_ARG without ffq_pair_set_merge): the
 * round's merged text is written as BGZF members on the device (ffq_stream_set_compress's way; each mate's own text is its
 * stream's business) and ffq_pair_merged_bgzf hands out the members and {bytes in, bytes out, members, members stored};
 * ffq_pair_merged then returns *h_text = NULL and keeps its counts.
 * ffq_pair_set_dedup (before the first ffq_pair_next only; FFQ_E_ARG if either stream has a dedup of its own -- ffq_pair_open
 * refuses such a stream, too): the pair owns one ffq_dedup; both mates' fronts take their keys over the round's window, on
 * the rows as scanned, and behind ffq_table_select_pairs, in front of the merge, the kept pairs are entered by their PAIR
 * keys with both tables compacted in step.  *n_pairs_out, ffq_pair_rows and h_index follow it; pairs[0] of
 * ffq_pair_selected keeps meaning "pairs the filter kept".  ffq_pair_dedup_counts: as ffq_stream_dedup_counts, in pairs,
 * over every round so far.
 * ffq_pair_set_correct (before the first ffq_pair_next only; FFQ_E_ARG afterwards, for rules out of range and without
 * ffq_pair_set_overlap; NULL switches it off, as does ffq_pair_set_overlap(NULL)): every round runs ffq_table_pair_correct on
 * both fills' device bytes, between the overlap and ffq_table_select_pairs, with the insert sizes the round's overlap pass
 * found.  The order of a round is then ends, quality, poly-G, adapter, poly-X, overlap, CORRECT, filter, dedup, merge.  Statistics IN
 * and the dedup keys are taken in front of the correction, on the bytes as read; the content filter, statistics OUT, the
 * render, the merge and the deflate see the corrected bytes.  ffq_pair_rows' h_bytes remain the bytes AS READ (the pinned
 * host copy is not corrected): a caller that cuts records from them itself does not see the corrections -- the rendered text
 * does.  ffq_pair_corrected: counts (NULL: not wanted) = the six counts of the last round, matrix (NULL: not wanted) = the
 * corrections of every round so far by kind, as ffq_table_pair_correct lays them out.  FFQ_E_ARG without ffq_pair_set_correct.
 * Not done: interleaved input or output, paired readfastq_iter_range.                                                  */
typedef struct ffq_pair ffq_pair;
int  ffq_pair_open(ffq_stream *mate1, ffq_stream *mate2, int pair_filter, int check_names, ffq_pair **out);
int  ffq_pair_wants(ffq_pair *p);
int  ffq_pair_next(ffq_pair *p, int64_t *n_pairs_in, int64_t *n_pairs_out, int *end_state, int *err_mate, int64_t *err_offset);
int  ffq_pair_rows(ffq_pair *p, int mate, const int64_t **h_rows, const uint8_t **h_bytes, int64_t *n_bytes, int64_t *bytes_offset);
int  ffq_pair_selected(ffq_pair *p, const int64_t **h_index, int64_t pairs[5]);
int  ffq_pair_set_overlap(ffq_pair *p, const ffq_overlap_rules *rules);
int  ffq_pair_overlap(ffq_pair *p, int64_t counts[FFQ_OVERLAP_COUNTS], uint64_t *h_hist, int64_t cap_words);
int  ffq_pair_set_merge(ffq_pair *p, int on);
int  ffq_pair_merged(ffq_pair *p, const uint8_t **h_text, int64_t *n_bytes, int64_t counts[FFQ_MERGE_COUNTS]);
int  ffq_pair_set_compress(ffq_pair *p, int mode);
int  ffq_pair_merged_bgzf(ffq_pair *p, const uint8_t **h_bgzf, int64_t *n_bytes, int64_t stats[FFQ_DEFLATE_COUNTS]);
int  ffq_pair_set_dedup(ffq_pair *p, int drop, int64_t expected_keys, int64_t max_bytes);
int  ffq_pair_dedup_counts(ffq_pair *p, int64_t counts[FFQ_DEDUP_COUNTS]);
/* UMIs of a pair (before the first ffq_pair_next): the names check still compares the headers as read; the take runs in the
 * front of the mate or mates rules->loc names; BOTH mates' renders put the same insert into their names, each tag read from
 * the kept rows of the mate that carries it (a pair whose named mate -- with _PER_READ: either of them -- is too short for
 * a tag gets none).  FFQ_E_ARG with merging switched on, and ffq_pair_set_merge behind it: the merged read's header is not
 * tagged.  ffq_pair_umi_counts: ffq_stream_umi_counts of either mate for the round ffq_pair_next has just returned.      */
int  ffq_pair_set_umi(ffq_pair *p, const ffq_umi_rules *rules);
int  ffq_pair_umi_counts(ffq_pair *p, int64_t counts1[4], int64_t counts2[4]);
int  ffq_pair_set_correct(ffq_pair *p, const ffq_correct_rules *rules);
int  ffq_pair_corrected(ffq_pair *p, int64_t counts[FFQ_CORRECT_COUNTS], int64_t matrix[FFQ_CORRECT_MATRIX_WORDS]);
void ffq_pair_close(ffq_pair *p);

/* Bytes [pos, pos + n_bytes) of the file behind fd into device memory (read(), fastqandfurious.py:30-36, for a range
 * that stays resident): pread in slices by the context's helper threads into pinned slots, each slot over the link in
 * two halves on two copy streams while the next is read.  Returns when the bytes are in d_dst; *n_loaded < n_bytes:
 * the file ended there.  The descriptor's position is not moved.  The helper threads (FFQ_POOL_THREADS, default 16) run
 * on the CPUs next to the GPU (/sys/bus/pci/devices/<bdf>/local_cpulist within the process's own affinity) and the
 * pinned slots are allocated from there: on a two-socket host the other socket costs a fifth of the rate
 * (FFQ_POOL_AFFINITY=0: nothing is bound; FFQ_POOL_DEBUG=1 says what was done).                                   */
int  ffq_load_fd(ffq_ctx *ctx, int fd, int64_t pos, int64_t n_bytes, void *d_dst, int64_t *n_loaded);

/* ---- synthetic FASTQ generators (bench / test inputs) -----
 * Counter-based (splitmix64), so the numpy generator in
 * fastq-and-furious_amd/synth.py produces the same bytes.
 * S-single: record i = "@SYN.%010d/1\n" + 150 bases + "\n+\n" + 150 quals +
 * "\n" = 322 bytes.  Writes records [first, first+count) at d_out.          */
int ffq_synth_single(ffq_ctx *ctx, uint8_t *d_out, int64_t first, int64_t count,
                     uint64_t seed);
/* S-wrapped: lengths 50..300, 80-column wrap, '+' line repeats the header
 * for one record in four.  d_start[i] (int64, count+1 entries, relative to
 * d_out) must hold the exclusive prefix sum of ffq_synth_wrapped_size().     */
int64_t ffq_synth_wrapped_size(int64_t i, uint64_t seed);
int ffq_synth_wrapped(ffq_ctx *ctx, uint8_t *d_out, const int64_t *d_start,
                      int64_t first, int64_t count, uint64_t seed);

/* ---- diagnostics ---------------------------------------------------------
 * Runs the device self-checks (wave scan, newline mask) and returns FFQ_OK.  */
int ffq_selftest(ffq_ctx *ctx);

/* ---- one stream over the GPUs of a node: byte-range shards ------------------------------------
 * Rank r of `world` owns the stream bytes [bounds[r], bounds[r + 1]) and every record whose '@' lies in
 * them; offsets count from bounds[0] (readfastq_iter's globaloffset, /root/reference/src/fastqandfurious.py
 * :198-242).  What the reference does with a record that does not fit its buffer -- keep buf[offset:] and
 * read more (:274-279) -- happens per range edge.  One process per GPU, one ffq_shard per process; the
 * hand-offs are RCCL over xGMI (librccl, loaded at run time):
 *   ffq_shard_unique_id   rank 0 draws the communicator id (ncclGetUniqueId); the host hands the 128 bytes
 *                         to every rank (MPI, torch.distributed, a file ...)
 *   ffq_shard_create      every rank, collectively (ncclCommInitRank, twice: hand-offs and the gather have
 *                         a communicator each)
 *   ffq_shard_halo        how many bytes in front of / behind its range this rank's buffer holds:
 *                         d_ext = [tail | own bytes | head], tail = min(tail_bytes, lo - bounds[0]),
 *                         head = min(head_bytes, bounds[world] - hi); the caller fills the middle
 *   ffq_shard_step_submit one step, queued, no host wait: the halos from the ranks that own them
 *                         (ncclSend / ncclRecv in one group; overlap_handoff != 0: on the shard's hand-off
 *                         stream, beside whatever the scan stream is doing -- the caller vouches that no
 *                         scan in flight reads d_ext, e.g. every lane has a buffer of its own), the scan of
 *                         the whole view, the rows of the range cut out (as ffq_table_cut) and ONE
 *                         ncclAllGather of eight words per rank
 *   ffq_shard_step_wait   the step's result: rows [row_lo, row_hi) of d_table are this rank's records
 *                         (absolute stream offsets), record_base their global ordinal; exit_pos (first
 *                         record start at / behind my right edge) equals the right neighbour's first_pos
 *                         on return -- that, with rank 0's exact start, proves every range.  A look-ahead
 *                         that ends inside the straddling record is grown (d_ext in the result then points
 *                         at the shard's own, larger view), a contradicted entry guess re-entered from the
 *                         left neighbour's exit: `rounds` counts those.  err_state != 0: the stream's error
 *                         (FFQ_END_ERR_*, the byte the reference's ValueError names in err_byte), the same
 *                         on every rank.  FFQ_E_TABLE_FULL (on every rank) if some rank's table is too small
 *                         (scan.n_records = the rows that rank's view holds) or, decoding, its quality buffer
 *                         (scan.n_records = 0, scan.n_qual_bytes = the bytes needed).
 *   ffq_shard_create_lane a second shard of the same rank on another context (ffq_ctx_create_shared: same
 *                         scan stream), on the first one's communicators: steps queued one ahead.
 *   ffq_shard_world_* / ffq_shard_create_local   k logical ranks as THREADS of one process on one GPU, hand-offs
 *                         by device copies (tests, dry runs): every rank's thread makes the same calls.
 * Every rank must make the same sequence of calls (they are collective).
 *
 * A step cannot hang silently (round 6).  WATCHDOG: every wait of a step -- ffq_shard_step_wait, the in-process
 * barrier -- polls with a deadline (FFQ_SHARD_TIMEOUT_S, default 30 s, 0 = none; ffq_shard_set_timeout); when it
 * runs out the call returns FFQ_E_TIMEOUT and ffq_last_error names the STAGE the step is stuck in (hand-off / scan /
 * gather), the transport, the mode and -- as far as this rank can see them -- the ranks whose words have and have not
 * arrived; RCCL's own asynchronous errors (ncclCommGetAsyncError) end the wait at once.  After FFQ_E_TIMEOUT the shard is
 * poisoned: ffq_shard_abort (ncclCommAbort on its communicators, its streams drained) and ffq_shard_destroy are what is
 * left; the host may then build a new one.  SERIAL MODE: the pipelined step drives TWO communicators from THREE streams
 * (hand-off of step i + 1 beside the scan of step i, the gather behind it); the serial step is ONE communicator on ONE
 * stream -- hand-off, scan, words, gather in order on the scan stream (lanes share it) -- the same rows, nothing
 * overlapped: the fallback a host takes once after a watchdog trip (FFQ_SHARD_SERIAL=1 at creation -- the second
 * communicator is then never made --, or ffq_shard_set_serial between steps).  ffq_shard_result.serial / .nranks and
 * ffq_shard_get_info say what ran.                                                                            */
#define FFQ_SHARD_STAGE_NONE    0
#define FFQ_SHARD_STAGE_HANDOFF 1
#define FFQ_SHARD_STAGE_SCAN    2
#define FFQ_SHARD_STAGE_GATHER  3
#define FFQ_SHARD_MAX_INFO_RANKS 64
typedef struct ffq_shard ffq_shard;
typedef struct ffq_shard_world ffq_shard_world;
typedef struct ffq_shard_result {
    ffq_scan_result scan;      /* the local scan of [tail | own | head]                                    */
    int64_t n_rows;            /* rows it wrote to d_table                                                  */
    int64_t row_lo, row_hi;    /* this rank's records                                                       */
    int64_t exit_pos, first_pos;   /* stream offsets; -1: none (the view reaches the end of the stream)     */
    int64_t n_own_records, record_base, total_records;
    int64_t err_byte;
    int32_t err_state;         /* 0, or FFQ_END_ERR_*                                                       */
    int32_t rounds;            /* repair rounds (0: the first scan of every rank stood)                     */
    int32_t regathers;         /* gathers repeated because some rank's scan needed a later tier             */
    int32_t halo_source;       /* 0: the halos were handed off between ranks; 1: read from the file (ffq_shard_load_fd) */
    int64_t handoff_bytes;     /* bytes this rank sent + received in hand-offs                              */
    float   handoff_ms;        /* device time of the halo hand-off (events on the stream it ran on)         */
    float   allgather_ms;      /* device time of the gather(s) of the eight words                           */
    uint8_t *d_ext;            /* the view the rows refer to (the caller's, or a grown one owned by the shard) */
    int64_t tail, head;
    int32_t nranks;            /* ranks of the communicator the words were gathered on (ncclCommCount; == world) */
    int32_t serial;            /* 1: the serial step ran (one communicator, one stream), 0: the pipelined one   */
    int64_t n_slabs;           /* ffq_shard_scan_fd_slabs: slabs the range went through (re-reads included); else 0 */
    int64_t bytes_read;        /* ... and the bytes it read from the file                                        */
} ffq_shard_result;
/* Who is there: filled at creation (RCCL: ncclCommCount of both communicators and ONE all-gather of every rank's PCI
 * bus id, so that a host can assert "N ranks on N distinct GPUs" before it trusts a number).                     */
typedef struct ffq_shard_info {
    int32_t rank, world;
    int32_t nranks_handoff;    /* ncclCommCount of the hand-off communicator (other transports: world)          */
    int32_t nranks_gather;     /* ... of the gather communicator; 0: there is none (created serial)             */
    int32_t serial;            /* the mode the next step runs in                                                */
    int32_t last_stage;        /* FFQ_SHARD_STAGE_*: where the last watchdog trip found the step (0: no trip)   */
    int32_t poisoned;          /* 1: a watchdog trip or an asynchronous RCCL error: only abort / destroy are left */
    int32_t n_bus;             /* entries of bus_id that are filled: min(world, FFQ_SHARD_MAX_INFO_RANKS)       */
    double  timeout_s;         /* the watchdog's deadline (0: none)                                             */
    int64_t bus_id[FFQ_SHARD_MAX_INFO_RANKS];   /* PCI domain << 16 | bus << 8 | device << 3 | function of rank r's GPU; -1: unknown
                                                   (in-process / hosted transports know their own only)        */
} ffq_shard_info;
int  ffq_shard_unique_id(uint8_t *id128);
int  ffq_shard_create(ffq_ctx *ctx, const uint8_t *id128, int rank, int world, const int64_t *bounds,
                      int64_t tail_bytes, int64_t head_bytes, ffq_shard **out);
/* ... with the mode said by the caller instead of the environment (mode: FFQ_SHARD_F_*) */
#define FFQ_SHARD_F_SERIAL 1u
int  ffq_shard_create2(ffq_ctx *ctx, const uint8_t *id128, int rank, int world, const int64_t *bounds,
                       int64_t tail_bytes, int64_t head_bytes, uint32_t mode, ffq_shard **out);
int  ffq_shard_create_lane(ffq_shard *parent, ffq_ctx *ctx, ffq_shard **out);
int  ffq_shard_world_create(int world, ffq_shard_world **out);
void ffq_shard_world_abort(ffq_shard_world *w);
void ffq_shard_world_destroy(ffq_shard_world *w);
int  ffq_shard_create_local(ffq_ctx *ctx, ffq_shard_world *w, int rank, const int64_t *bounds, int64_t tail_bytes,
                            int64_t head_bytes, ffq_shard **out);
void ffq_shard_destroy(ffq_shard *s);
int  ffq_shard_halo(ffq_shard *s, int64_t *tail, int64_t *head);
int  ffq_shard_exchange_halo(ffq_shard *s, uint8_t *d_ext, int overlap);
int  ffq_shard_step_submit(ffq_shard *s, uint8_t *d_ext, int overlap_handoff, uint32_t flags, int qual_add,
                           int64_t *d_table, int64_t table_cap, int8_t *d_qual, int64_t qual_cap, int64_t *d_qoff);
int  ffq_shard_step_wait(ffq_shard *s, ffq_shard_result *out);
const char *ffq_shard_transport(ffq_shard *s);    /* "rccl" / "in-process" / "hosted" */
int  ffq_shard_get_info(ffq_shard *s, ffq_shard_info *out);
int  ffq_shard_set_timeout(ffq_shard *s, double seconds);      /* the watchdog's deadline (every lane of the rank) */
int  ffq_shard_set_serial(ffq_shard *s, int on);               /* between steps, no lane pending; every rank alike */
/* After FFQ_E_TIMEOUT (or at any time): ncclCommAbort on the shard's communicators -- kernels of a collective that
 * waits for a peer leave --, an injected stall released, the shard's streams drained with a deadline of their own.
 * FFQ_OK: drained; FFQ_E_TIMEOUT: something still runs (ffq_shard_destroy then leaks the shard's device memory
 * rather than wait for ever) -- in particular ncclCommAbort ITSELF, which runs on a thread of its own with a deadline
 * (FFQ_SHARD_ABORT_S, default 30 s) here: with a peer whose process is gone RCCL's teardown waits on its sockets for
 * minutes and holds the device's runtime meanwhile (every other HIP call of the process waits behind it); the caller
 * has its error in time and should leave with _exit.  The same wait meets a rank that aborts AFTER its peers have
 * torn their ends down: the ranks' deadlines do not run out at the same instant, so a host lets them MEET over its
 * own control plane first and abort together (sharded.abort_together: a barrier on the process group, then this
 * call; a peer that never reports fails the meeting and nothing is aborted).  Only ffq_shard_destroy may follow. */
int  ffq_shard_abort(ffq_shard *s);
/* diagnostics: the NEXT step of this shard hangs at `stage` (FFQ_SHARD_STAGE_*) for up to `seconds` -- a one-lane
 * kernel on that stage's stream that waits for a host flag (released by ffq_shard_abort / _destroy) -- so that the
 * watchdog and the recovery can be exercised without a broken peer (tests/test_watchdog.py).                   */
int  ffq_shard_inject_stall(ffq_shard *s, int stage, double seconds);
/* A shard of a FILE: bounds[] are file offsets.  ffq_shard_load_fd reads this rank's bytes [lo - tail, hi + head) of fd
 * (pread: the descriptor's position is not moved) into d_ext -- helper threads -> pinned slots -> hipMemcpyAsync on two
 * copy streams -- and returns when they are there; a step submitted over that d_ext then hands off NOTHING between
 * ranks (the halos are the file's own bytes: ffq_shard_result.halo_source = 1), and a look-ahead that has to grow is
 * read from the file by the rank that needs it.  The gather of the eight words, and with it the proof of every range
 * and the global ordinals, is unchanged.  Every rank of the world or none (the ranks must agree on whether a grown
 * look-ahead is an exchange).  fd < 0: detach (steps hand off between ranks again).  This is what replaces the
 * reference's single reader per rank: read() (fastqandfurious.py:30-36), the first fill and its sentinel (:241-245,
 * rank 0's view starts the stream), the carry of an unfinished entry (:274-279, here the look-ahead).           */
int  ffq_shard_load_fd(ffq_shard *s, int fd, uint8_t *d_ext, int64_t *n_bytes);
/* ... and a range that does NOT fit the GPU (a 2 TB file over eight of them): the same step with this rank's view going
 * through ONE device buffer of slab_bytes, slab after slab -- what the reference's loop does for any size of stream: scan
 * the buffer, keep the unfinished entry, read more (fastqandfurious.py:251-279).  Slab k + 1 begins at the byte the search
 * of slab k stopped at (the iterator's `offset`: exact, no guess between slabs), its rows go behind slab k's in d_table
 * (rows [0, n_rows): all of the pass, [row_lo, row_hi) this rank's, absolute file offsets), the bytes are dropped.  At the
 * rank's two edges nothing changes: the entry guessed from the run-in, eight words, one gather, the same decision; a rank
 * whose guess its left neighbour's chain contradicts streams its range again from that neighbour's exit; a look-ahead that
 * must grow is read on; one record longer than the slab doubles the slab.  Collective like a step (every rank calls it, or
 * ffq_shard_step_* over a loaded range: the words are the same).  No FFQ_F_DECODE_QUAL.  FFQ_E_TABLE_FULL (every rank):
 * scan.n_records = an estimate of the rows that rank's view needs.  d_ext of the result is NULL: nothing stays resident. */
int  ffq_shard_scan_fd_slabs(ffq_shard *s, int fd, int64_t slab_bytes, uint32_t flags, int64_t *d_table, int64_t table_cap,
                             ffq_shard_result *out);
/* The same step over HOST memory with the transport supplied by the caller (and, for tests, the scan): the protocol
 * functions are the device step's (csrc/ffq_shard_proto.h), driven synchronously.  For hosts whose ranks cannot talk RCCL
 * -- a multi-process CPU test-suite over gloo (scan = the test's own engine), a functional dry run of several ranks on
 * one GPU (scan = NULL: ffq_scan_host on `ctx`) -- not a CPU fallback: without a scan callback it needs a context like
 * every other compute entry point.
 *   exchange   collective: the same list of pieces on every rank; for a piece with src == rank, ptr is where its b - a
 *              bytes are read from, with dst == rank where they go (NULL on ranks that are neither)
 *   allgather  collective: SH words (8 x int64) of every rank into all[world][8]
 *   scan       ffq_scan_host's contract over h_buf (rows + add into h_table, res filled; FFQ_E_TABLE_FULL with
 *              res->n_records = the need)
 * h_ext = [tail | own bytes | head] with the middle filled (ffq_shard_halo's sizes from the same bounds and byte counts);
 * on return out->d_ext is the view the rows refer to: h_ext, or a larger one the step allocated (a look-ahead had to
 * grow) that the caller releases with ffq_shard_host_free.  Callbacks return 0 or a negative FFQ_E_* code.          */
typedef struct ffq_shard_piece { int32_t src, dst; int64_t a, b; uint8_t *ptr; } ffq_shard_piece;
typedef struct ffq_shard_host_ops {
    void *user;
    int (*scan)(void *user, const uint8_t *h_buf, int64_t n_bytes, int sentinel, int64_t offset, int eof, int64_t add,
                int64_t *h_table, int64_t table_cap, ffq_scan_result *res);
    int (*exchange)(void *user, const ffq_shard_piece *pieces, int n_pieces);
    int (*allgather)(void *user, const int64_t *mine, int64_t *all);
} ffq_shard_host_ops;
/* ... and the DEVICE step (ffq_shard_step_*: buffers in HBM, the scan and the words on the device) over the caller's
 * transport: hand-offs staged through host memory around ops->exchange, the words gathered by ops->allgather (ops->scan is
 * not used; the callbacks and `user` must stay valid while the shard lives).  ffq_shard_transport says "hosted".  For ranks
 * that cannot talk RCCL -- several processes sharing ONE GPU, a group over gloo / MPI; with file-backed shards
 * (ffq_shard_load_fd) the only traffic is the 64 bytes of words per rank.                                            */
int  ffq_shard_create_hosted(ffq_ctx *ctx, const ffq_shard_host_ops *ops, int rank, int world, const int64_t *bounds,
                             int64_t tail_bytes, int64_t head_bytes, ffq_shard **out);
int  ffq_shard_host_step(const ffq_shard_host_ops *ops, ffq_ctx *ctx, int rank, int world, const int64_t *bounds,
                         int64_t tail_bytes, int64_t head_bytes, uint8_t *h_ext, int64_t *h_table, int64_t table_cap,
                         ffq_shard_result *out);
void ffq_shard_host_free(void *p);
/* diagnostics: n bytes from d_src to d_dst through the shard's transport with this rank at both ends */
int  ffq_shard_self_exchange(ffq_shard *s, const uint8_t *d_src, uint8_t *d_dst, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* FFQ_H */
