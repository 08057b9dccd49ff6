"""Host-side mirror of the reference module `fastqandfurious.fastqandfurious`
for the FASTQ hot path (reference: /root/reference/src/fastqandfurious.py).

Same names, argument order, status constants and exception texts as the
reference, so code written against it runs unchanged:

    from fastqandfurious_amd import fastqandfurious, _fastqandfurious
    for header, sequence, quality in fastqandfurious.readfastq_iter(
            fh, fbufsize, fastqandfurious.entryfunc, _fastqandfurious.entrypos):
        ...

`entrypos` below is the pure-Python plug-in scanner of the reference
(:39-100) -- the CPU-only configuration of BASELINE.json -- written from its
documented behaviour.  `_fastqandfurious.entrypos` is the MI355X scanner; when
readfastq_iter is handed a scanner that exposes `scan_buffer` it parses every
record of a buffer fill with ONE batched GPU call instead of one call per
record, and yields exactly the same entries.

Beyond the hot path: the FASTA plug-in scanner of the reference
(`entrypos_fasta`, `entryfunc_fasta`, :103-143, :174-183) and a working `automagic_open`
(:282-334; the reference's own cannot run: it calls `importlib.importmodule` and ignores its
`openers` argument).
"""
from array import array
from collections import namedtuple
from functools import partial
import importlib
from itertools import islice, repeat
import os
import typing

import numpy as np

from . import entries as _entries
from . import hip as _hip

CHAR_AT: int = ord(b'@')
CHAR_PLUS: int = ord(b'+')
CHAR_NEWLINE: int = ord(b'\n')
BYTES_NEWLINE_AT: bytes = b'\n@'
BYTES_NEWLINE_PLUS: bytes = b'\n+'
CHAR_GT: int = ord(b'>')
BYTES_NEWLINE_GT: bytes = b'\n>'
ARRAY_INIT = array('q', [-1, ] * 6)

Entry = namedtuple('Entry', 'header sequence quality')
EntryType = typing.Tuple[bytes, bytes, typing.Optional[bytes]]

# status codes, reference :19-27
INVALID: int = -1
MISSING_SEQHEADER_BEGIN: int = 0
MISSING_SEQHEADER_END: int = 1
MISSING_SEQ_BEG: int = 2
MISSING_SEQ_END: int = 3
MISSING_QUAL_BEGIN: int = 4
MISSING_QUAL_END: int = 5
COMPLETE: int = 6
MISSING_QUALHEADER_END: int = 7

# end states reported by a batched scanner (include/ffq.h FFQ_END_*)
_END_OK, _END_REFILL, _END_ERR_FINAL_QUAL, _END_ERR_INCOMPLETE, _END_ERR_INVALID = range(5)


def read(fh: typing.BinaryIO, fbufsize: int) -> typing.Tuple[bytes, bool]:
    """One chunk of the stream and whether it was the last one.

    Reference :30-36: end of stream is signalled by a short read."""
    blob = fh.read(fbufsize)
    return (blob, len(blob) < fbufsize)


def entrypos(buf: bytes, offset: int, posbuffer) -> int:
    """Pure-Python scanner: positions of the next FASTQ entry in `buf`.

    Behaviour of the reference's Python `entrypos` (:39-100): searches with
    bytes.find, fills posbuffer[0..5] as far as it gets (earlier content is
    left in place, there is no reset) and returns a status code.
    """
    size = len(buf)
    nl_at = buf.find(BYTES_NEWLINE_AT, offset)
    if nl_at < 0:
        return MISSING_SEQHEADER_BEGIN
    posbuffer[0] = nl_at + 1
    head_end = buf.find(b'\n', nl_at + 2)
    if head_end < 0:
        return MISSING_SEQHEADER_END
    posbuffer[1] = head_end
    seq_beg = head_end + 1
    if seq_beg >= size:
        return MISSING_SEQ_BEG
    posbuffer[2] = seq_beg
    seq_end = buf.find(BYTES_NEWLINE_PLUS, seq_beg)
    if seq_end < 0:
        return MISSING_SEQ_END
    posbuffer[3] = seq_end
    plus_end = buf.find(b'\n', seq_end + 2)
    if plus_end < 0:
        return MISSING_QUALHEADER_END
    plus_line = plus_end - seq_end          # '+' line incl. its newline
    if plus_line - 1 > 1 and plus_line != head_end - nl_at:
        return INVALID                      # '+' line carries text of another length
    qual_beg = plus_end + 1
    if qual_beg >= size:
        return MISSING_QUAL_BEGIN
    posbuffer[4] = qual_beg
    qual_end = qual_beg + (seq_end - seq_beg)
    if qual_end + 2 >= size:
        return MISSING_QUAL_END
    posbuffer[5] = qual_end
    return COMPLETE


def entrypos_fasta(buf: bytes, offset: int, posbuffer) -> int:
    """Plug-in scanner for FASTA (reference :103-143): next "\\n>" from `offset`, end of the
    header line, then the sequence up to the next "\\n>".  Fills posbuffer[0..3] as far as
    it gets and returns MISSING_SEQHEADER_BEGIN / _END, MISSING_SEQ_BEG, MISSING_SEQ_END (the
    buffer ended first: posbuffer[3] is then the end of the buffer, without a trailing
    newline) or COMPLETE."""
    i = buf.find(BYTES_NEWLINE_GT, offset)
    if i < 0:
        return MISSING_SEQHEADER_BEGIN
    posbuffer[0] = i + 1
    j = buf.find(b'\n', i + 2)
    if j < 0:
        return MISSING_SEQHEADER_END
    posbuffer[1] = j
    if j + 1 >= len(buf):
        return MISSING_SEQ_BEG
    posbuffer[2] = j + 1
    k = buf.find(BYTES_NEWLINE_GT, j + 1)
    if k < 0:
        posbuffer[3] = len(buf) - 1 if buf[-1] == CHAR_NEWLINE else len(buf)
        return MISSING_SEQ_END
    posbuffer[3] = k
    return COMPLETE


def entryfunc_fasta(buf: bytes, pos, globaloffset: int):
    """(header, sequence) byte slices of a FASTA entry (reference :174-183)."""
    return (buf[(pos[0] + 1):pos[1]], buf[pos[2]:pos[3]])


def entryfunc_namedtuple(buf: bytes, pos, globaloffset: int) -> Entry:
    """Entry(header, sequence, quality) namedtuple (reference :146-158)."""
    return Entry(buf[(pos[0] + 1):pos[1]], buf[pos[2]:pos[3]], buf[pos[4]:pos[5]])


def entryfunc(buf: bytes, pos, globaloffset: int) -> EntryType:
    """(header, sequence, quality) byte slices (reference :161-171)."""
    return (buf[(pos[0] + 1):pos[1]], buf[pos[2]:pos[3]], buf[pos[4]:pos[5]])


_ENTRYFUNC = entryfunc          # (readfastq_iter's parameter shadows the name)


def entryfunc_phred(buf: bytes, pos, globaloffset: int):
    """(header, sequence, quality) with the quality as an array('b') of Phred scores: the entryfunc the
    reference's user guide writes for this (doc/user-guide.rst:126-141, :206-214; benchmark.py:155-168),

        quality = array('b'); quality.frombytes(buf[pos[4]:pos[5]]); arrayadd_b(quality, -33)

    Called per record (any scanner) it does exactly that, through this package's arrayadd_b -- one
    device round trip per record.  readfastq_iter RECOGNISES it when the scanner is the GPU one: the
    stream front end then decodes the qualities of a whole buffer fill on the device, together with
    the scan (FFQ_F_DECODE_QUAL, k_decode_stream), and the iterator only wraps the decoded bytes --
    the same entries, without a call per record."""
    from . import _fastqandfurious as _C
    quality = array('b')
    quality.frombytes(buf[pos[4]:pos[5]])
    _C.arrayadd_b(quality, -33)
    return (buf[(pos[0] + 1):pos[1]], buf[pos[2]:pos[3]], quality)


class entryfunc_lengthfilter:
    """The length filter of the reference's user guide (doc/user-guide.rst:153-180) as an entryfunc OBJECT:

        LENGTH_THRESHOLD = 25
        def lengthfilter_entryfunc(buf, posarray):
            if posarray[3] - posarray[2] < LENGTH_THRESHOLD:
                return buf[posarray[2]:posarray[3]]
            else:
                return None

    is entryfunc_lengthfilter(25): called per record (any scanner; with or without the third argument the iterator
    passes, :255) it does exactly that -- the sequence of a read SHORTER than the threshold, None for the others; the
    iterator yields one item per record either way.  More generally min_len <= pos[3] - pos[2] <= max_len is kept
    (the length is the byte length of the slice, as in the guide: a wrapped read counts its newlines), and `column`
    says what is built for a kept record: "sequence" (the guide's), "header", "quality", or "entry" -- the (header,
    sequence, quality) tuple of entryfunc.

    readfastq_iter RECOGNISES the object when the scanner is the GPU one: the stream front end filters every buffer
    fill's offset table on the device, gathers the one component of the kept rows there (ffq_stream_set_filter), and
    copies back nothing of a dropped record -- for which the iterator then spends one None in a list instead of a
    scanner call, an entryfunc call and three slices.  Same items, same order.

    yield_dropped=False (an extension: the guide's loop skips the Nones itself, `if sequence is None: # do nothing`):
    the iterator yields the kept records' items only -- a dropped record then never reaches the interpreter at all."""

    def __init__(self, threshold=None, min_len=None, max_len=None, column="sequence", yield_dropped=True):
        if column not in ("sequence", "header", "quality", "entry"):
            raise ValueError("column must be 'sequence', 'header', 'quality' or 'entry'")
        if threshold is not None:
            if max_len is not None:
                raise ValueError("threshold and max_len say the same thing")
            max_len = int(threshold) - 1
        self.min_len = None if min_len is None else int(min_len)
        self.max_len = None if max_len is None else int(max_len)
        self.column = column
        self.yield_dropped = bool(yield_dropped)

    def keeps(self, length):
        return (self.min_len is None or length >= self.min_len) and (self.max_len is None or length <= self.max_len)

    def __call__(self, buf, pos, globaloffset=None):
        if not self.keeps(pos[3] - pos[2]):
            return None
        c = self.column
        if c == "sequence":
            return buf[pos[2]:pos[3]]
        if c == "header":
            return buf[(pos[0] + 1):pos[1]]
        if c == "quality":
            return buf[pos[4]:pos[5]]
        return (buf[(pos[0] + 1):pos[1]], buf[pos[2]:pos[3]], buf[pos[4]:pos[5]])


def _trim_end(d):
    """Bases the running-sum rule takes off the end that `d` = cutoff - (q - base) is walked from: the walk stops when the
    sum goes negative; the cut is behind the FIRST maximum of the sums in front of that, if it is above 0."""
    c = np.cumsum(d)
    neg = np.flatnonzero(c < 0)
    if neg.size:
        c = c[:neg[0]]
    if not c.size:
        return 0
    k = int(np.argmax(c))               # (the first maximum)
    return k + 1 if c[k] > 0 else 0


def quality_trim_span(quality, cutoff_back, cutoff_front=0, qual_base=33):
    """(start, stop) of the quality-trimmed read within `quality` (bytes of one record's quality line): the running-sum
    rule of BWA's and cutadapt's -q, either end with its own cutoff and independent of the other (include/ffq.h,
    ffq_table_trim_quality, states it as a loop).  A read that is trimmed away is (0, 0)."""
    n = len(quality)
    if n == 0:
        return 0, 0
    q = np.frombuffer(quality, dtype=np.uint8).astype(np.int64) - qual_base
    start = _trim_end(cutoff_front - q)
    stop = n - _trim_end(cutoff_back - q[::-1])
    return (start, stop) if start < stop else (0, 0)


def trimmable(buf, pos):
    """Does the device trim this row (ffq_table_trim_quality's eligibility)?  pos2..pos5 inside `buf`, sequence and
    quality of one length, no newline in the quality (a wrapped record)."""
    p2, p3, p4, p5 = pos[2], pos[3], pos[4], pos[5]
    return (p2 >= 0 and p4 >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
            and b'\n' not in buf[p4:p5])


class entryfunc_qualitytrim:
    """Quality trimming as an entryfunc OBJECT -- the other use the reference's user guide names for a table of positions
    (doc/user-guide.rst:196-204: "trimming either end of the read could be done by ... modifying the values in a table of
    indices"): the running-sum rule of BWA / cutadapt -q (quality_trim_span) moves pos2..pos5 of the record inwards, a read
    whose trimmed length is outside [min_len, max_len] gives None, any other the component `column` says ("entry": the
    (header, sequence, quality) tuple of entryfunc; "sequence", "quality", "header") cut at the trimmed positions.  A
    record the rule does not apply to (wrapped lines, sequence and quality of different lengths) is left as it is.

    Called per record (any scanner) it works on a copy of `pos`: the caller's posbuffer is not touched.  readfastq_iter
    RECOGNISES the unmodified class when the scanner is the GPU one: the stream front end then trims every fill's table
    on the device right behind the scan (ffq_stream_set_trim), drops what became too short there and gathers the one
    component of the kept rows (ffq_stream_set_filter) -- no quality string reaches the interpreter to be trimmed.  Same
    items, same order, one per record."""

    yield_dropped = True

    def __init__(self, cutoff_back, cutoff_front=0, qual_base=33, min_len=None, max_len=None, column="entry"):
        if column not in ("sequence", "header", "quality", "entry"):
            raise ValueError("column must be 'sequence', 'header', 'quality' or 'entry'")
        if not (0 <= int(cutoff_back) <= 127 and 0 <= int(cutoff_front) <= 127):
            raise ValueError("cutoffs are 0..127")
        if not 0 <= int(qual_base) <= 255:
            raise ValueError("qual_base is 0..255")
        self.cutoff_back, self.cutoff_front, self.qual_base = int(cutoff_back), int(cutoff_front), int(qual_base)
        self.min_len = None if min_len is None else int(min_len)
        self.max_len = None if max_len is None else int(max_len)
        self.column = column

    def trimmed_pos(self, buf, pos):
        """A copy of the six positions with the rule applied."""
        pos = list(pos)
        if trimmable(buf, pos):
            start, stop = quality_trim_span(buf[pos[4]:pos[5]], self.cutoff_back, self.cutoff_front, self.qual_base)
            pos[2], pos[3], pos[4], pos[5] = pos[2] + start, pos[2] + stop, pos[4] + start, pos[4] + stop
        return pos

    def __call__(self, buf, pos, globaloffset=None):
        pos = self.trimmed_pos(buf, pos)
        length = pos[3] - pos[2]
        if (self.min_len is not None and length < self.min_len) or (self.max_len is not None and length > self.max_len):
            return None
        c = self.column
        if c == "sequence":
            return buf[pos[2]:pos[3]]
        if c == "header":
            return buf[(pos[0] + 1):pos[1]]
        if c == "quality":
            return buf[pos[4]:pos[5]]
        return (buf[(pos[0] + 1):pos[1]], buf[pos[2]:pos[3]], buf[pos[4]:pos[5]])


def _adapter_args(adapter, err_permille, min_overlap):
    """(adapter as bytes, err_permille, min_overlap) or ValueError: the ranges ffq_table_trim_adapter takes."""
    adapter = bytes(adapter)
    if not 1 <= len(adapter) <= 64:
        raise ValueError("the adapter has 1..64 bytes")
    if not 1 <= int(min_overlap) <= len(adapter):
        raise ValueError("min_overlap is 1..len(adapter)")
    if not 0 <= int(err_permille) <= 1000:
        raise ValueError("err_permille is 0..1000")
    return adapter, int(err_permille), int(min_overlap)


def adapter_cut(sequence, adapter, err_permille=100, min_overlap=3):
    """Length that is left of `sequence` (bytes of one record's sequence line) when it is cut at the 3' adapter: the LEFTMOST
    position p <= len(sequence) - min_overlap at which the first ov = min(len(adapter), len(sequence) - p) bytes of the
    adapter differ from sequence[p:p + ov] in at most ov * err_permille // 1000 places -- a full copy inside the read or a
    prefix of the adapter at its end; b'N' in the adapter matches anything, bytes are compared as they are, no indels
    (include/ffq.h, ffq_table_trim_adapter, states it as a loop; cutadapt -a AD --no-indels -e E -O O takes the best-scoring
    position where this takes the leftmost).  len(sequence) if there is none."""
    adapter, err, mo = _adapter_args(adapter, err_permille, min_overlap)
    n, m = len(sequence), len(adapter)
    if n < mo:
        return n
    ncand = n - mo + 1
    pos = np.arange(ncand, dtype=np.int64)
    seq = np.concatenate((np.frombuffer(sequence, dtype=np.uint8), np.zeros(m, dtype=np.uint8)))
    mm = np.zeros(ncand, dtype=np.int64)
    for j, a in enumerate(adapter):
        if a != 0x4E:
            mm += (seq[j:j + ncand] != a) & (pos + j < n)
    hit = np.flatnonzero(mm <= np.minimum(m, n - pos) * err // 1000)
    return int(hit[0]) if hit.size else n


def adapter_trimmable(buf, pos):
    """Does the device cut this row at an adapter (ffq_table_trim_adapter's eligibility)?  trimmable()'s rule with the newline
    looked for in the SEQUENCE."""
    p2, p3, p4, p5 = pos[2], pos[3], pos[4], pos[5]
    return (p2 >= 0 and p4 >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
            and b'\n' not in buf[p2:p3])


_POLY_BASES = _hip.POLY_BASES


def _poly_min_len(name, min_len):
    """min_len of a poly pass as an int (None: the pass is off) or ValueError naming the setting: the range ffq_table_trim_poly takes."""
    if min_len is None:
        return None
    lo, hi = _hip.POLY_MIN_LEN
    if isinstance(min_len, bool) or not isinstance(min_len, (int, np.integer)) or not lo <= int(min_len) <= hi:
        raise ValueError("%s is None or %d..%d" % (name, lo, hi))
    return int(min_len)


def poly_tail_cut(sequence, base=None, min_len=10):
    """Length that is left of `sequence` (bytes of one record's sequence line) when its poly tail is cut off: the host
    statement of ffq_table_trim_poly's rule (include/ffq.h states it as a loop).  base: b"A", b"C", b"G" or b"T" -- poly-G is
    b"G" --, or None for any of the four (poly-X).  The read is walked from its 3' end; per base of the set, the positions that
    are not that base (either case; N and every other byte match nothing) are counted, and the walk stops at the first position
    i >= min_len - 1 at which every base of the set has more than min(5, (i + 1) // 8) of them.  A walk that got to min_len
    positions cuts the read behind the deepest exact copy of the base with the most hits; len(sequence) otherwise."""
    if base not in _POLY_BASES:
        raise ValueError('base is b"A", b"C", b"G", b"T" or None')
    min_len = _poly_min_len("min_len", min_len)
    if min_len is None:
        raise ValueError("min_len is 2..65535")
    n = len(sequence)
    if n < min_len:
        return n
    k = _BASE_CLASS[np.frombuffer(sequence, dtype=np.uint8)[::-1]]           # classes in walk order
    bases = range(4) if base is None else (_POLY_BASES[base],)
    i = np.arange(n)
    allowed = np.minimum(5, (i + 1) // 8)
    failing = i >= min_len - 1
    for b in bases:
        failing &= np.cumsum(k != b) > allowed
    at = np.flatnonzero(failing)
    stop = int(at[0]) if at.size else n
    if stop < min_len:
        return n
    hits = [int(np.count_nonzero(k[:stop] == b)) for b in bases]
    best = bases[hits.index(max(hits))]                                      # (ties: the lowest class)
    where = np.flatnonzero(k[:stop] == best)
    return n - 1 - (int(where[-1]) if where.size else -1)


def poly_trimmable(buf, pos):
    """Does the device cut a poly tail off this row (ffq_table_trim_poly's eligibility)?  adapter_trimmable's rule."""
    return adapter_trimmable(buf, pos)


def _poly_pos(buf, pos, base, min_len):
    """(the six positions -- a list, edited in place -- with the rule applied, bases cut)"""
    if not poly_trimmable(buf, pos):
        return pos, 0
    n = pos[3] - pos[2]
    cut = poly_tail_cut(buf[pos[2]:pos[3]], base, min_len)
    pos[3], pos[5] = pos[2] + cut, pos[4] + cut
    return pos, n - cut


class UmiRules:
    """Where a read's unique molecular identifier is and how it goes into the name (`fastp --umi --umi_loc --umi_len --umi_skip
    --umi_prefix`; include/ffq.h states the rule, which follows fastp's documented behaviour and has not been checked against
    its source).  loc: "read1", "read2" or "per_read" -- the mate whose first `length` (1..64) bases are the UMI, or both;
    skip (0..64): bases dropped behind it; the name gets delim (one printable byte) + prefix + b"_" (prefix: 0..16 bytes of
    [A-Za-z0-9], nothing of this if empty) + the UMI (per_read: both, with b"_" between) in front of its first blank.
    ValueError names the setting that is out of range."""

    def __init__(self, loc="read1", length=8, skip=0, prefix=b"", delim=b":"):
        self.loc, self.length, self.skip, self.prefix, self.delim = loc, length, skip, prefix, delim
        self._check()

    def _check(self):
        def whole(x, lo, hi):
            return not isinstance(x, bool) and isinstance(x, (int, np.integer)) and lo <= int(x) <= hi
        if self.loc not in _hip.UMI_LOCS:
            raise ValueError('loc is "read1", "read2" or "per_read"')
        if not whole(self.length, 1, _hip.UMI_LEN_MAX):
            raise ValueError("length is 1..%d" % _hip.UMI_LEN_MAX)
        if not whole(self.skip, 0, _hip.UMI_SKIP_MAX):
            raise ValueError("skip is 0..%d" % _hip.UMI_SKIP_MAX)
        if not isinstance(self.prefix, (bytes, bytearray)) or len(self.prefix) > _hip.UMI_PREFIX_MAX or \
                not all(48 <= b <= 57 or 65 <= b <= 90 or 97 <= b <= 122 for b in self.prefix):
            raise ValueError("prefix is 0..%d bytes of [A-Za-z0-9]" % _hip.UMI_PREFIX_MAX)
        if not isinstance(self.delim, (bytes, bytearray)) or len(self.delim) != 1 or not 0x21 <= self.delim[0] <= 0x7E:
            raise ValueError("delim is one printable byte (0x21..0x7E)")
        self.length, self.skip, self.prefix, self.delim = int(self.length), int(self.skip), bytes(self.prefix), bytes(self.delim)

    def takes(self, mate):
        """does mate 1 or 2 lose bases?"""
        return self.loc == "per_read" or self.loc == ("read1", "read2")[mate - 1]


def umi_take(sequence, quality, rules):
    """(the UMI or None, sequence, quality) of one ELIGIBLE read (umi_takable) with its UMI taken off: the host statement of
    ffq_table_take_umi's rule.  A read shorter than rules.length keeps its bases and gives None; any other loses
    min(length + skip, len) bases at its 5' end, and may go to length 0."""
    n = len(sequence)
    if n < rules.length:
        return None, sequence, quality
    cut = min(rules.length + rules.skip, n)
    return bytes(sequence[:rules.length]), sequence[cut:], quality[cut:]


def umi_name(header, tags, rules):
    """`header` (bytes, as entryfunc cuts it) with the insert in front of its first b" " or b"\t", at its end if it has none:
    the host statement of ffq_table_render_fastq_umi's rule.  tags: the UMI, or the two of "per_read" (mate 1's first)."""
    k = len(header)
    for blank in (b" ", b"\t"):
        at = header.find(blank, 0, k)
        if at >= 0:
            k = at
    return b"".join((header[:k], rules.delim, rules.prefix + b"_" if rules.prefix else b"", b"_".join(tags), header[k:]))


def umi_takable(buf, pos):
    """Does the device take a UMI off this row (ffq_table_take_umi's eligibility)?  adapter_trimmable's rule, no newline in
    the quality either, and the sequence begins right behind the header's newline (a scanned, unwrapped record)."""
    return adapter_trimmable(buf, pos) and b'\n' not in buf[pos[4]:pos[5]] and pos[2] == pos[1] + 1


def _umi_pos(buf, pos, rules):
    """(the six positions -- a list, edited in place -- with the UMI taken, the UMI or None, was the row skipped)"""
    if not umi_takable(buf, pos):
        return pos, None, True
    n = pos[3] - pos[2]
    if n < rules.length:
        return pos, None, False
    tag = bytes(buf[pos[2]:pos[2] + rules.length])
    cut = min(rules.length + rules.skip, n)
    pos[2] += cut
    pos[4] += cut
    return pos, tag, False


class UmiReport:
    """What filter_fastq(umi=..., umi_report=...) and filter_fastq_paired fill, the same on either route: reads_tagged (records
    WRITTEN with a UMI in their name, both outputs of a pair counted), bases_removed (UMI and skipped bases, over every record
    read), reads_skipped (records the take does not apply to: wrapped records)."""

    def __init__(self):
        self.reads_tagged = self.bases_removed = self.reads_skipped = 0

    def _add_counts(self, counts):
        """(rows taken, bases removed, rows skipped, rows tagged in the output) (hip: umi_counts)"""
        self.bases_removed += counts[1]
        self.reads_skipped += counts[2]
        self.reads_tagged += counts[3]


def _check_umi(umi, umi_report, single, merging=False):
    """filter_fastq's / filter_fastq_paired's umi and umi_report, checked before anything is opened or read; the report to fill"""
    if umi is not None:
        if not isinstance(umi, UmiRules):
            raise TypeError("umi must be a UmiRules")
        try:
            umi._check()
        except ValueError as e:
            raise ValueError("umi: %s" % e) from None
        if single and umi.loc != "read1":
            raise ValueError('umi: a single file has read 1 only (loc is "read1")')
        if merging:
            raise ValueError("umi does not go with merged_out: a merged read's name is not tagged")
    if umi_report is not None and umi is None:
        raise ValueError("umi_report needs umi")
    if umi_report is not None and not isinstance(umi_report, UmiReport):
        raise TypeError("umi_report must be a UmiReport")
    return _report(umi_report, UmiReport)


class EndRules:
    """What ffq_table_trim_ends does to both ends of a read, in front of every other trim (include/ffq.h states the rule):
    trim_front / trim_tail bases go from the 5' / 3' end whatever they are (`fastp -f / -t`, `cutadapt -u`), keep_len (None: no
    limit) is the most that is then left, the 3' end giving way (`fastp -b`, `cutadapt -l`); front, right and tail are each None
    or (window, quality), window 1..64 and quality 1..93: the sliding windows of `fastp --cut_front / --cut_right / --cut_tail`
    (-5 / -r / -3) and of Trimmomatic's SLIDINGWINDOW (`right`), which cut where the mean quality of `window` bases drops
    below `quality`.  At least one of the six is on."""

    WINDOW_MAX = _hip.ENDS_WINDOW_MAX
    QUALITY = _hip.ENDS_QUALITY

    def __init__(self, trim_front=0, trim_tail=0, keep_len=None, front=None, right=None, tail=None):
        def count(name, x, none_ok=False):
            if x is None and none_ok:
                return None
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < 1 << 31:
                raise ValueError("ends: %s is %san int >= 0" % (name, "None or " if none_ok else ""))
            return int(x)

        def window(name, st):
            if st is None:
                return None
            try:
                w, q = st
            except (TypeError, ValueError):
                raise ValueError("ends: %s is None or (window, quality)" % name) from None
            for x in (w, q):
                if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
                    raise ValueError("ends: %s is None or (window, quality), two ints" % name)
            if not 1 <= int(w) <= self.WINDOW_MAX:
                raise ValueError("ends: the window of %s is 1..%d" % (name, self.WINDOW_MAX))
            if not self.QUALITY[0] <= int(q) <= self.QUALITY[1]:
                raise ValueError("ends: the quality of %s is %d..%d" % ((name,) + self.QUALITY))
            return int(w), int(q)
        self.trim_front, self.trim_tail = count("trim_front", trim_front), count("trim_tail", trim_tail)
        self.keep_len = count("keep_len", keep_len, True) or None
        self.front, self.right, self.tail = window("front", front), window("right", right), window("tail", tail)
        if not (self.trim_front or self.trim_tail or self.keep_len or self.front or self.right or self.tail):
            raise ValueError("ends: every rule is off")


def _check_ends(ends):
    """an EndRules or None; ValueError naming `ends` for anything else"""
    if ends is not None and not isinstance(ends, EndRules):
        raise ValueError("ends must be an EndRules or None, not %r" % (ends,))
    return ends


def _ends_qual_base(qual_base):
    if not 0 <= int(qual_base) <= 255:
        raise ValueError("qual_base is 0..255")
    return int(qual_base)


def ends_cut(quality, rules, qual_base=33):
    """(a, b): what is left of a read whose quality line is `quality` (bytes) when `rules` (an EndRules) are applied -- the host
    statement of ffq_table_trim_ends's rule (include/ffq.h states it as a loop), here with prefix sums over the whole line.
    (0, 0) for a read that goes away."""
    if not isinstance(rules, EndRules):
        raise ValueError("rules must be an EndRules")
    qual_base = _ends_qual_base(qual_base)
    n = len(quality)
    a = min(rules.trim_front, n)
    b = n - min(rules.trim_tail, n - a)
    if rules.keep_len and b - a > rules.keep_len:
        b = a + rules.keep_len
    v = np.frombuffer(bytes(quality), dtype=np.uint8).astype(np.int64) - qual_base
    csum = np.concatenate((np.zeros(1, dtype=np.int64), np.cumsum(v)))

    def sums(w):                                          # S(i, w) for i = a .. b - w
        return csum[a + w:b + 1] - csum[a:b - w + 1]
    if rules.front is not None and b > a:
        w, q = min(rules.front[0], b - a), rules.front[1]
        at = np.flatnonzero(sums(w) >= q * w)
        if not at.size:
            return 0, 0
        a += int(at[0])
        a += int(np.flatnonzero(v[a:a + w] >= q)[0])
    if rules.right is not None and b > a:
        w, q = min(rules.right[0], b - a), rules.right[1]
        at = np.flatnonzero(sums(w) < q * w)
        if at.size:
            s = a + int(at[0])
            bad = np.flatnonzero(v[s:s + w] < q)
            b = s + (int(bad[0]) if bad.size else w)
    if rules.tail is not None and b > a:
        w, q = min(rules.tail[0], b - a), rules.tail[1]
        at = np.flatnonzero(sums(w) >= q * w)
        if not at.size:
            return 0, 0
        e = a + int(at[-1]) + w
        b = e - w + int(np.flatnonzero(v[e - w:e] >= q)[-1]) + 1
    return (a, b) if a < b else (0, 0)


def ends_trimmable(buf, pos):
    """Does the device apply an EndRules to this row (ffq_table_trim_ends's eligibility)?  trimmable()'s rule: the newline is
    looked for in the whole quality line."""
    return trimmable(buf, pos)


def _ends_pos(buf, pos, rules, qual_base):
    """(the six positions -- a list, edited in place -- with the rule applied, bases cut)"""
    if not ends_trimmable(buf, pos):
        return pos, 0
    n = pos[5] - pos[4]
    a, b = ends_cut(buf[pos[4]:pos[5]], rules, qual_base)
    pos[2], pos[3], pos[4], pos[5] = pos[2] + a, pos[2] + b, pos[4] + a, pos[4] + b
    return pos, n - (b - a)


def _report(given, cls):
    """The report a plan fills, which it then always has: the caller's -- reset in place, not added to -- or, given None, a
    private one of `cls`.  Every report fills from the count vectors hip returns, with one _add_counts (_from_counts: totals)."""
    if given is None:
        return cls()
    if isinstance(given, cls):
        given.__init__()                         # (a subclass resets what it added)
    else:
        given.__dict__.update(cls().__dict__)    # (overlap, merge, correction: any object will do, as it did)
    return given


class EndsReport:
    """What filter_fastq / filter_fastq_paired (ends_report=...) fill: reads_cut, the reads the ends step (EndRules) changed,
    and bases_cut, the bases it removed.  Both mates of a pair are added together; every record counts, the dropped ones
    included.  The same numbers on either route."""

    def __init__(self):
        self.reads_cut = self.bases_cut = 0

    def _add_counts(self, counts):
        """(rows changed, bases removed, ...) of the ends step (hip: ends_trimmed)"""
        self.reads_cut += counts[0]
        self.bases_cut += counts[1]


class PolyReport:
    """What filter_fastq / filter_fastq_paired (poly_report=...) fill: poly_g_reads and poly_g_bases, the reads the poly-G step
    changed and the bases it removed; poly_x_reads and poly_x_bases, the same for poly-X.  Both mates of a pair are added
    together; every record counts, the dropped ones included.  The same numbers on either route."""

    def __init__(self):
        self.poly_g_reads = self.poly_g_bases = self.poly_x_reads = self.poly_x_bases = 0

    def _add_counts(self, counts):
        """((rows changed, bases removed, ...) by poly-G, the same by poly-X) (hip: poly_trimmed)"""
        g, x = counts
        self.poly_g_reads += g[0]
        self.poly_g_bases += g[1]
        self.poly_x_reads += x[0]
        self.poly_x_bases += x[1]


class entryfunc_adaptertrim:
    """3' adapter trimming as an entryfunc OBJECT, beside entryfunc_qualitytrim: what `cutadapt [-q CUTOFF] -a ADAPTER
    --no-indels -e E -O O` does to a record.  The quality rule first if quality_cutoff is given (an int -- the 3' end -- or a
    (front, back) pair), then the read as that left it is cut at the adapter (adapter_cut); a read whose trimmed length is
    outside [min_len, max_len] gives None, any other the component `column` says, cut at the trimmed positions.  A record a
    rule does not apply to (trimmable / adapter_trimmable: wrapped lines, sequence and quality of different lengths) is left
    as that rule found it.

    Called per record (any scanner) it works on a copy of `pos`.  readfastq_iter RECOGNISES the unmodified class when the
    scanner is the GPU one: the stream front end trims every fill's table on the device (ffq_stream_set_trim,
    ffq_stream_set_adapter), filters it and gathers the one component of the kept rows.  Same items, same order, one per
    record.  Paired-end files: filter_fastq_paired (an adapter per mate, or none named: its `overlap`).  Not done: 5' and
    anchored adapters, indels, several adapters, readfastq_iter_range."""

    yield_dropped = True

    def __init__(self, adapter, err_permille=100, min_overlap=3, quality_cutoff=None, qual_base=33, min_len=None, max_len=None,
                 column="entry"):
        if column not in ("sequence", "header", "quality", "entry"):
            raise ValueError("column must be 'sequence', 'header', 'quality' or 'entry'")
        self.adapter, self.err_permille, self.min_overlap = _adapter_args(adapter, err_permille, min_overlap)
        self.quality = None
        if quality_cutoff is not None:
            front, back = (0, quality_cutoff) if isinstance(quality_cutoff, (int, np.integer)) else quality_cutoff
            self.quality = entryfunc_qualitytrim(back, front, qual_base)        # (checks the ranges)
        self.min_len = None if min_len is None else int(min_len)
        self.max_len = None if max_len is None else int(max_len)
        self.column = column

    def trimmed_pos(self, buf, pos):
        """A copy of the six positions with the rules applied."""
        pos = self.quality.trimmed_pos(buf, pos) if self.quality is not None else list(pos)
        if adapter_trimmable(buf, pos):
            cut = adapter_cut(buf[pos[2]:pos[3]], self.adapter, self.err_permille, self.min_overlap)
            pos[3], pos[5] = pos[2] + cut, pos[4] + cut
        return pos

    __call__ = entryfunc_qualitytrim.__call__


def entryfunc_abspos(buf: bytes, pos, globaloffset: int):
    """Absolute stream positions: pos[i] += globaloffset, in place; returns
    the same `pos` object (reference :186-195)."""
    for i in range(6):
        pos[i] += globaloffset
    return pos


_raise_for_end = _hip.raise_for_end


_ENTRY_CHUNK = 1024     # rows per native call: the tuples of one chunk are consumed (and their memory
                        # reused) before the next is built -- a whole fill at once is 3 x slower


def _pushes_down(entryfunc):
    """Is this entryfunc the library's own length filter, unchanged?  Only then may the device evaluate it from min_len /
    max_len / column alone; a subclass that overrides __call__ or keeps() is CALLED per record like any other entryfunc --
    on every scanner alike (the same entryfunc must not yield different items depending on the scanner)."""
    if not isinstance(entryfunc, entryfunc_lengthfilter):
        return False
    t = type(entryfunc)
    return t is entryfunc_lengthfilter or (t.__call__ is entryfunc_lengthfilter.__call__ and
                                           getattr(t, "keeps", None) is getattr(entryfunc_lengthfilter, "keeps", None))


def _pushes_down_trim(entryfunc):
    """... and its own quality trimmer, unchanged (a subclass with a __call__ or trimmed_pos of its own is called per record)."""
    if not isinstance(entryfunc, entryfunc_qualitytrim):
        return False
    t = type(entryfunc)
    return t is entryfunc_qualitytrim or (t.__call__ is entryfunc_qualitytrim.__call__ and
                                          t.trimmed_pos is entryfunc_qualitytrim.trimmed_pos)


def _pushes_down_adapter(entryfunc):
    """... and its own adapter trimmer, unchanged."""
    if not isinstance(entryfunc, entryfunc_adaptertrim):
        return False
    t = type(entryfunc)
    return t is entryfunc_adaptertrim or (t.__call__ is entryfunc_adaptertrim.__call__ and
                                          t.trimmed_pos is entryfunc_adaptertrim.trimmed_pos)


def _table_entries(entryfunc, buf, rows, shift, quals=None):
    """What readfastq_iter yields for one table, as an iterable of iterables (every front does `yield from` each): `rows` is
    C-contiguous int64, six stream positions per record (array('q') or ndarray); stream byte x is buf[x - shift], `buf` any
    buffer.  quals: None, or a callable giving the table's bulk Phred decode (qual, qoff) -- record i's bytes are
    qual[qoff[i] : qoff[i] + pos5 - pos4], packed stream and single-pass segments alike -- for entryfunc_phred.

    The bulk paths (entryfunc_phred over a decode, the default entryfunc and entryfunc_namedtuple) hand over one LIST per
    _ENTRY_CHUNK rows, cut natively (csrc/ffq_entries.c) straight out of `buf` where the module is built -- a generator
    level less per record.  Any other entryfunc is CALLED per record, lazily (not for record k + 1 before record k has been
    handed out), with what the reference's loop passes (:252-255): `buf` as bytes, a fresh array('q') of six
    buffer-relative positions, and `shift` as globaloffset; a length filter that is not pushed down and does not yield its
    dropped records has its Nones left out."""
    if not len(rows):
        return ()
    mv = memoryview(rows).cast('B')
    nat = _entries.native()
    step = 48 * _ENTRY_CHUNK
    if quals is not None and entryfunc is entryfunc_phred:
        qual, qoff = quals()
        if nat is not None and hasattr(nat, "entries_phred"):
            mo = memoryview(qoff).cast('B')
            return (nat.entries_phred(buf, mv[at:at + step], shift, qual, mo[at // 6:(at + step) // 6 + 8], array)
                    for at in range(0, len(mv), step))
        buf, qb, offs = bytes(buf), qual.tobytes(), qoff.tolist()
        rel = (np.frombuffer(mv, dtype=np.int64).reshape(-1, 6) - shift).tolist()
        return ([(buf[p0 + 1:p1], buf[p2:p3], array('b', qb[offs[i]:offs[i] + p5 - p4]))
                 for i, (p0, p1, p2, p3, p4, p5) in enumerate(rel)],)
    if (entryfunc is _ENTRYFUNC or entryfunc is entryfunc_namedtuple) and nat is not None:
        cls = None if entryfunc is _ENTRYFUNC else Entry
        return (nat.entries(buf, mv[at:at + step], shift, 1, cls) for at in range(0, len(mv), step))
    if not isinstance(buf, bytes):
        buf = bytes(buf)
    rel = array('q')
    rel.frombytes((np.frombuffer(mv, dtype=np.int64) - shift).tobytes())
    if entryfunc is _ENTRYFUNC:
        # the default entryfunc inlined: the same three slices per record (:161-171) without a posbuffer object and a
        # call per record (1.7 x the entries per second; a list of lists from tolist() is slower than either)
        it = iter(rel)
        z = zip(it, it, it, it, it, it)
        return iter(lambda: [(buf[p0 + 1:p1], buf[p2:p3], buf[p4:p5]) for p0, p1, p2, p3, p4, p5 in islice(z, _ENTRY_CHUNK)], [])
    out = _called(entryfunc, buf, rel, shift)
    if isinstance(entryfunc, entryfunc_lengthfilter) and not entryfunc.yield_dropped:
        return ((e for e in chunk if e is not None) for chunk in out)
    return out


_POS = tuple(slice(i, i + 6) for i in range(0, 6 * _ENTRY_CHUNK, 6))       # where the records of a chunk lie among its positions


def _called(entryfunc, buf, rel, shift):
    """entryfunc(buf, pos, shift) for every six positions of `rel` (array('q')), one lazy `map` per _ENTRY_CHUNK records: the
    call for a record is made when the front asks for its item, and nothing per record runs in the interpreter but the
    entryfunc itself (a generator level per record costs a tenth of the rate, slices built per record a twentieth)."""
    for at in range(0, len(rel), 6 * _ENTRY_CHUNK):
        part = rel[at:at + 6 * _ENTRY_CHUNK]
        yield map(entryfunc, repeat(buf), map(part.__getitem__, _POS[:len(part) // 6]), repeat(shift))


def _phred_entries(st, fill, rows, shift):
    """entryfunc_phred over a whole table, from the stream's bulk decode of that fill."""
    return _table_entries(entryfunc_phred, fill, rows, shift, st.quals)


def _kept_items(yield_dropped, n_items, where, col=None, off=None, buf=None, rows=None, shift=0):
    """The pushed-down length filter's items for n_items records of which the device kept len(where): a list with kept
    record j's item at where[j] and None elsewhere -- or, yield_dropped False, the kept records' items alone.  The item is
    col[off[j] : off[j + 1]] of the gathered column, or, col None ("entry"), the (header, sequence, quality) of row j of
    `rows` cut out of `buf` (positions minus `shift` index it)."""
    k = len(where)
    if not yield_dropped:                       # as if every record had been kept
        n_items, where = k, np.arange(k, dtype=np.int64)
    if k == 0:
        return [None] * n_items
    nat = _entries.native()
    if col is None:
        if nat is not None and hasattr(nat, "sparse_entries"):
            return nat.sparse_entries(n_items, memoryview(where).cast('B'), buf, memoryview(rows).cast('B'), shift)
        out, buf = [None] * n_items, bytes(buf)
        for j, (p0, p1, p2, p3, p4, p5) in zip(where.tolist(), (rows - shift).tolist()):
            out[j] = (buf[p0 + 1:p1], buf[p2:p3], buf[p4:p5])
        return out
    if nat is not None and hasattr(nat, "sparse"):
        return nat.sparse(n_items, memoryview(where).cast('B'), col, memoryview(off).cast('B'))
    out, cb, o = [None] * n_items, col.tobytes(), off.tolist()
    for j, at in enumerate(where.tolist()):
        out[at] = cb[o[j]:o[j + 1]]
    return out


def _cut_column(buf, rows, shift, column):
    """(bytes uint8[], offsets int64[n + 1]) of one component ("header" as entryfunc cuts it, "sequence", "quality") of
    every row, cut out of `buf` (positions minus `shift` index it) in one numpy gather: FileShard.kept_column on the host."""
    ca, shf, cb = _hip.Context.COLUMNS[column]
    beg, lens = rows[:, ca] + shf - shift, np.maximum(rows[:, cb] - rows[:, ca] - shf, 0)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    src = np.repeat(beg - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
    return np.frombuffer(buf, dtype=np.uint8)[src], off


def iter_tables(fh, fbufsize, scan_buffer):
    """One (buf, rows, globaloffset) per buffer fill that holds a record, with a batched scanner:
    scan_buffer(buf, offset, eof) -> (rows, end_state, end_offset) where rows is an array('q') of 6*n
    buffer-relative positions, `rows[i] + globaloffset` the absolute ones.  The refill, the sentinel,
    globaloffset and the error texts follow the reference loop (:241-279) step for step."""
    globaloffset = -1
    offset = 0
    buf, eof = read(fh, fbufsize)
    buf = b'\n' + buf
    while True:
        rows, end_state, end_offset = scan_buffer(buf, offset, eof)
        if len(rows):
            yield buf, rows, globaloffset
        offset = end_offset
        if end_state == _END_OK:
            return
        if end_state != _END_REFILL:
            _raise_for_end(end_state, globaloffset + offset)
        globaloffset += offset
        tmp_buf, eof = read(fh, fbufsize)
        buf = buf[offset:] + tmp_buf
        del tmp_buf
        offset = 0


def _iter_batched(fh, fbufsize, entryfunc, scan_buffer):
    """readfastq_iter with a batched scanner: one scan per buffer fill (iter_tables)."""
    # a scanner may name a number of bytes below which reads are coalesced into k * fbufsize per scan
    # (the entries do not depend on where the stream is cut into fills)
    co = getattr(getattr(scan_buffer, '__self__', None), 'coalesce_bytes', 0) or 0
    if 0 < fbufsize < co:
        fbufsize *= -(-co // fbufsize)
    for buf, rows, globaloffset in iter_tables(fh, fbufsize, scan_buffer):
        for chunk in _table_entries(entryfunc, buf, np.frombuffer(rows, dtype=np.int64) + globaloffset, globaloffset):
            yield from chunk


def _iter_stream(st, entryfunc):
    """readfastq_iter over the native stream front end (ffq_stream_*): the library reads the
    file (ahead, into pinned memory), scans every buffer fill and hands back the rows; this loop
    only builds the entries, out of the stream's own (pinned) fill."""
    try:
        for rows, fill, fill_offset, end_state, err_offset in st:
            if st.filtered:
                # the stream dropped rows on the device (entryfunc_lengthfilter): one item per scanned record all the same
                idx, n_scanned, col, off = st.selected()
                yield from _kept_items(entryfunc.yield_dropped, n_scanned, idx, col, off, fill, rows, fill_offset)
            else:
                for chunk in _table_entries(entryfunc, fill, rows, fill_offset, st.quals if st.decode else None):
                    yield from chunk
            if end_state != _END_OK and end_state != _END_REFILL:
                _raise_for_end(end_state, err_offset)
    finally:
        st.close()


def readfastq_iter(fh: typing.BinaryIO, fbufsize: int,
                   entryfunc: typing.Callable = entryfunc,
                   entrypos: typing.Callable = entrypos,
                   globaloffset: int = 0) -> typing.Iterator[EntryType]:
    """Iterate through entries in a FASTQ stream (reference :198-279).

    :param fh: anything with a `read(n)` method returning bytes
    :param fbufsize: chunk size of the reads from `fh`
    :param entryfunc: builds the yielded object from (buf, pos, globaloffset)
    :param entrypos: scanner (buf, offset, posbuffer) -> status
    :param globaloffset: accepted and ignored, as in the reference (:242)

    Differences from the reference, both on malformed input only: an INVALID
    entry met after the end of the stream raises 'Entry is invalid at byte'
    (the reference never leaves its loop, :256-270).
    """
    open_stream = getattr(entrypos, 'open_stream', None)
    if open_stream is not None:
        # the native stream front end: a real file, a gzip file, or anything with readinto() / read();
        # with entryfunc_phred the qualities of every fill are decoded on the device
        st = open_stream(fh, fbufsize, entryfunc is entryfunc_phred) if entryfunc is entryfunc_phred else open_stream(fh, fbufsize)
        if st is not None and (_pushes_down(entryfunc) or _pushes_down_trim(entryfunc) or _pushes_down_adapter(entryfunc)
                               or _pushes_down_content(entryfunc)):
            # push-down: the filter runs on the device, on every fill's table, before anything is copied back -- behind the
            # quality and adapter trimming of the rows, if that is what the entryfunc does
            try:
                cutter = entryfunc if isinstance(entryfunc, entryfunc_adaptertrim) else None
                trim = cutter.quality if cutter is not None else entryfunc if isinstance(entryfunc, entryfunc_qualitytrim) else None
                content = entryfunc.rules if isinstance(entryfunc, entryfunc_contentfilter) else None
                _configure_stream(st, trim, cutter, content, (entryfunc.min_len, entryfunc.max_len),
                                  None if entryfunc.column == "entry" else entryfunc.column)
            except BaseException:
                st.close()                 # (the native stream, its pinned buffers and its feeder thread; a gzip stream's hook)
                raise
        if st is not None:
            yield from _iter_stream(st, entryfunc)
            return
    scan_buffer = getattr(entrypos, 'scan_buffer', None)
    if scan_buffer is not None:
        yield from _iter_batched(fh, fbufsize, entryfunc, scan_buffer)
        return

    if isinstance(entryfunc, entryfunc_lengthfilter) and not entryfunc.yield_dropped:
        # (the kept records only: the reference's loop below with the guide's `if sequence is None: # do nothing` folded in;
        # the object itself -- a subclass with a __call__ / keeps() of its own included -- with yield_dropped switched on)
        import copy
        keep_all = copy.copy(entryfunc)
        keep_all.yield_dropped = True
        yield from (e for e in readfastq_iter(fh, fbufsize, keep_all, entrypos) if e is not None)
        return
    posbuffer = array('q', [-1, ] * 6)
    globaloffset = -1
    offset = 0
    buf, eof = read(fh, fbufsize)
    buf = b'\n' + buf               # sentinel: the first '@' is then a "\n@" match
    while True:
        status = entrypos(buf, offset, posbuffer)
        if status == COMPLETE:
            offset = posbuffer[5] - 1
            yield entryfunc(buf, posbuffer, globaloffset)
            continue
        if eof:
            if status == MISSING_SEQHEADER_BEGIN:
                return
            if status == MISSING_QUAL_END:
                # last record of a stream: its quality may run to the last byte
                qualend = posbuffer[4] + (posbuffer[3] - posbuffer[2])
                if qualend >= len(buf):
                    raise ValueError('Incomplete final quality string at byte')
                posbuffer[5] = qualend
                yield entryfunc(buf, posbuffer, globaloffset)
                return
            if status == INVALID:
                raise ValueError('Entry is invalid at byte %i' % (globaloffset + offset))
            raise ValueError('Incomplete entry at byte %i' % (globaloffset + offset))
        if status == INVALID:
            raise ValueError('Entry is invalid at byte %i' % (globaloffset + offset))
        globaloffset += offset
        tmp_buf, eof = read(fh, fbufsize)
        buf = buf[offset:] + tmp_buf
        del tmp_buf
        offset = 0


def stats_eligible(buf, pos):
    """Does the device count this row (ffq_table_stats' eligibility)?  pos2..pos5 inside `buf`, sequence and quality of one
    length, no newline in either (a wrapped record)."""
    p2, p3, p4, p5 = pos[2], pos[3], pos[4], pos[5]
    return (p2 >= 0 and p4 >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
            and b'\n' not in buf[p2:p3] and b'\n' not in buf[p4:p5])


_BASE_CLASS = np.full(256, 4, dtype=np.int64)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _BASE_CLASS[list(_pair)] = _i


class FastqStats:
    """Per-cycle base and quality statistics of reads: the words ffq_table_stats counts (include/ffq.h has the layout),
    as named numpy uint64 views of one array `words` -- head (8), cycle_base (C x 5: A C G T other), cycle_qual (C x 96),
    len_hist (C + 1, the last bin "C or longer"), readq_hist (96, by a read's mean quality), gc_hist (101, by its GC per
    cent) -- with C = max_cycles.  This class is the host statement of the rule: add_record for one eligible record,
    add_rows for a table (rows the rule does not apply to count in head[1] only); from_words wraps what the device counted;
    += merges two of one shape (the ranks of a sharded read summing theirs).
    keyed, distinct, duplicates, duplication_rate: set by fastq_stats(duplication=True) only (DedupReport's fields)."""
    keyed = distinct = duplicates = duplication_rate = None

    def __init__(self, max_cycles=512, qual_base=33):
        max_cycles, qual_base = int(max_cycles), int(qual_base)
        if not 1 <= max_cycles <= _hip.STATS_MAX_CYCLES:
            raise ValueError("max_cycles is 1..%d" % _hip.STATS_MAX_CYCLES)
        if not 0 <= qual_base <= 255:
            raise ValueError("qual_base is 0..255")
        self.max_cycles, self.qual_base = max_cycles, qual_base
        self._view(np.zeros(_hip.stats_words(max_cycles), dtype=np.uint64))

    def _view(self, words):
        C = self.max_cycles
        self.words = words
        self.head = words[:8]
        self.cycle_base = words[8:8 + 5 * C].reshape(C, 5)
        self.cycle_qual = words[8 + 5 * C:8 + 101 * C].reshape(C, 96)
        self.len_hist = words[8 + 101 * C:8 + 102 * C + 1]
        self.readq_hist = words[8 + 102 * C + 1:8 + 102 * C + 97]
        self.gc_hist = words[8 + 102 * C + 97:]

    @classmethod
    def from_words(cls, words, max_cycles=512, qual_base=33):
        """The statistics the device counted: `words` (anything numpy reads as stats_words(max_cycles) uint64) is copied."""
        self = cls(max_cycles, qual_base)
        words = np.array(words, dtype=np.uint64).reshape(-1)
        if words.size != self.words.size:
            raise ValueError("%d words, max_cycles = %d has %d" % (words.size, self.max_cycles, self.words.size))
        self._view(words)
        return self

    def add_record(self, sequence, quality):
        """One eligible record: `sequence` and `quality` are bytes of one length without a newline."""
        n = len(sequence)
        if len(quality) != n:
            raise ValueError("sequence and quality differ in length")
        C, one = self.max_cycles, np.uint64(1)
        self.head[0] += one
        self.len_hist[min(n, C)] += one
        if n == 0:
            return
        cls_ = _BASE_CLASS[np.frombuffer(sequence, dtype=np.uint8)]
        v = np.clip(np.frombuffer(quality, dtype=np.uint8).astype(np.int64) - self.qual_base, 0, 95)
        m = min(n, C)
        cyc = np.arange(m)
        np.add.at(self.cycle_base, (cyc, cls_[:m]), one)
        np.add.at(self.cycle_qual, (cyc, v[:m]), one)
        sv, gc = int(v.sum()), int(np.count_nonzero((cls_ == 1) | (cls_ == 2)))
        self.head[2] += np.uint64(n)
        self.head[3] += np.uint64(n - m)
        self.head[4] += np.uint64(sv)
        self.head[5] += np.uint64(gc)
        self.head[6] += np.uint64(np.count_nonzero(cls_ == 4))
        self.readq_hist[sv // n] += one
        self.gc_hist[(100 * gc) // n] += one

    def add_pos(self, buf, pos):
        """One row of positions into `buf`: counted if the rule applies to it (stats_eligible), else skipped (head[1])."""
        if stats_eligible(buf, pos):
            self.add_record(buf[pos[2]:pos[3]], buf[pos[4]:pos[5]])
        else:
            self.head[1] += np.uint64(1)

    def add_rows(self, buf, rows, shift=0):
        """Every row of a table (int64 [n][6]; positions minus `shift` index `buf`)."""
        buf = bytes(buf) if not isinstance(buf, bytes) else buf
        for row in np.asarray(rows, dtype=np.int64).reshape(-1, 6):
            self.add_pos(buf, (row - shift).tolist())
        return self

    def __iadd__(self, other):
        if not isinstance(other, FastqStats):
            return NotImplemented
        if (other.max_cycles, other.qual_base) != (self.max_cycles, self.qual_base):
            raise ValueError("statistics of different max_cycles / qual_base do not add")
        self.words += other.words
        return self

    def __eq__(self, other):
        return (isinstance(other, FastqStats) and (other.max_cycles, other.qual_base) == (self.max_cycles, self.qual_base)
                and np.array_equal(self.words, other.words))

    __hash__ = None

    reads = property(lambda self: int(self.head[0]), doc="records counted")
    bases = property(lambda self: int(self.head[2]), doc="their bases")

    @property
    def gc_fraction(self):
        """G + C among all bases (NaN without bases)."""
        return float(self.head[5]) / self.bases if self.bases else float("nan")

    @property
    def mean_quality_per_cycle(self):
        """Mean quality value of every cycle (float64[max_cycles]; NaN where no read reaches)."""
        q = self.cycle_qual.astype(np.float64)
        tot = q.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (q * np.arange(96)).sum(axis=1) / tot

    def _rate(self, q):
        tot = int(self.cycle_qual.sum())
        return float(self.cycle_qual[:, q:].sum()) / tot if tot else float("nan")

    q20_rate = property(lambda self: self._rate(20), doc="share of the bases at cycles below max_cycles with quality >= 20")
    q30_rate = property(lambda self: self._rate(30), doc="... with quality >= 30")


# FFQ_EE_MICRO of include/ffq.h: floor(1e6 * 10 ** (-v / 10) + 0.5) for v = 0..95, the expected errors of a base of quality
# v in millionths -- the literals the library holds (ffq_ee_micro_table)
EE_MICRO = (1000000, 794328, 630957, 501187, 398107, 316228, 251189, 199526, 158489, 125893,
            100000, 79433, 63096, 50119, 39811, 31623, 25119, 19953, 15849, 12589,
            10000, 7943, 6310, 5012, 3981, 3162, 2512, 1995, 1585, 1259,
            1000, 794, 631, 501, 398, 316, 251, 200, 158, 126,
            100, 79, 63, 50, 40, 32, 25, 20, 16, 13,
            10, 8, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1, 1) + (0,) * 32
_EE_MICRO_NP = np.array(EE_MICRO, dtype=np.int64)


class ContentRules:
    """What a read is dropped for besides its length -- cutadapt's --max-n and --max-ee, fastp's -n, -e, -q / -u and -y -- as
    ffq_table_select_reads takes it (include/ffq.h states the rule; this class is its host statement).  With v[i] =
    clamp(quality[i] - qual_base, 0, 95), a read of n bases is dropped by the FIRST of these that fails:

        2 "n"                max_n: more than max_n bases are 'N' or 'n'
        3 "mean_quality"     min_mean_quality (1..95): sum(v) < min_mean_quality * n
        4 "unqualified"      max_unqualified_percent (0..100): 100 * #{v[i] < qualified_quality} > max_unqualified_percent * n
        5 "expected_errors"  max_expected_errors (a float, kept as millionths: max_ee_micro = int(round(x * 1e6))):
                             sum(EE_MICRO[v[i]]) > max_ee_micro
        6 "complexity"       min_complexity (1..100): n >= 2 and 100 * #{i < n - 1: seq[i] != seq[i + 1]} < min_complexity * (n - 1)

    (rule 1, "length", is the length filter's and is not this class's).  None switches a rule off.  A read of length 0
    passes all of them.  Integers throughout."""

    REASONS = ("length", "n", "mean_quality", "unqualified", "expected_errors", "complexity")

    def __init__(self, max_n=None, min_mean_quality=None, qualified_quality=15, max_unqualified_percent=None,
                 max_expected_errors=None, min_complexity=None, qual_base=33):
        def ranged(name, x, lo, hi, off):
            if x is None:
                return off
            x = int(x)
            if not lo <= x <= hi:
                raise ValueError("%s is %d..%d (None: off)" % (name, lo, hi))
            return x
        self.max_n = ranged("max_n", max_n, 0, (1 << 31) - 1, -1)
        self.min_mean_qual = ranged("min_mean_quality", min_mean_quality, 1, 95, 0)
        self.qualified_qual = ranged("qualified_quality", 15 if qualified_quality is None else qualified_quality, 0, 95, 15)
        self.max_unqualified_pct = ranged("max_unqualified_percent", max_unqualified_percent, 0, 100, -1)
        self.min_complexity_pct = ranged("min_complexity", min_complexity, 1, 100, 0)
        self.qual_base = ranged("qual_base", 33 if qual_base is None else qual_base, 0, 255, 33)
        if max_expected_errors is None:
            self.max_ee_micro = -1
        else:
            x = float(max_expected_errors)
            if not 0 <= x <= 9.0e12:              # (also refuses NaN)
                raise ValueError("max_expected_errors is a number of errors >= 0 (None: off)")
            self.max_ee_micro = int(round(x * 1e6))
        self._v = bytes(min(max(b - self.qual_base, 0), 95) for b in range(256))

    @property
    def active(self):
        """Is one of the rules switched on?"""
        return (self.max_n >= 0 or self.min_mean_qual > 0 or self.max_unqualified_pct >= 0 or self.max_ee_micro >= 0
                or self.min_complexity_pct > 0)

    def verdict(self, sequence, quality):
        """0 if the rules keep the read, else the number (2..6, REASONS[number - 1]) of the first rule that drops it.
        `sequence` and `quality` are bytes of one length."""
        n = len(sequence)
        if len(quality) != n:
            raise ValueError("sequence and quality differ in length")
        if n == 0:
            return 0
        if self.max_n >= 0 and sequence.count(b"N") + sequence.count(b"n") > self.max_n:
            return 2
        v = np.frombuffer(bytes(quality).translate(self._v), dtype=np.uint8)
        if self.min_mean_qual > 0 and int(v.sum(dtype=np.int64)) < self.min_mean_qual * n:
            return 3
        if self.max_unqualified_pct >= 0 and 100 * int(np.count_nonzero(v < self.qualified_qual)) > self.max_unqualified_pct * n:
            return 4
        if self.max_ee_micro >= 0 and int(_EE_MICRO_NP[v].sum()) > self.max_ee_micro:
            return 5
        if self.min_complexity_pct > 0 and n >= 2:
            s = np.frombuffer(sequence, dtype=np.uint8)
            if 100 * int(np.count_nonzero(s[1:] != s[:-1])) < self.min_complexity_pct * (n - 1):
                return 6
        return 0

    def verdict_pos(self, buf, pos):
        """(verdict, judged) of one row of positions into `buf`: a row the rules do not apply to (stats_eligible: a wrapped
        record, positions outside the buffer, lines of two lengths) is kept and not judged."""
        if not stats_eligible(buf, pos):
            return 0, False
        return self.verdict(buf[pos[2]:pos[3]], buf[pos[4]:pos[5]]), True


class entryfunc_contentfilter(entryfunc_lengthfilter):
    """entryfunc_lengthfilter that also drops a record for what is in it: `rules` is a ContentRules, applied to a record
    whose length min_len / max_len keep (rows the rules do not apply to -- wrapped records -- go by their length alone).
    The item is None for a dropped record and the `column` of a kept one; yield_dropped=False leaves the Nones out.

    readfastq_iter recognises the unchanged class when the scanner is the GPU one and judges every fill's rows on the
    device (ffq_stream_set_content + ffq_stream_set_filter); a subclass with a __call__ of its own is called per record.
    Same items, same order, with any scanner."""

    def __init__(self, rules, min_len=None, max_len=None, column="sequence", yield_dropped=True):
        if not isinstance(rules, ContentRules):
            raise TypeError("rules must be a ContentRules")
        super().__init__(None, min_len, max_len, column, yield_dropped)
        self.rules = rules

    def __call__(self, buf, pos, globaloffset=None):
        if not self.keeps(pos[3] - pos[2]) or self.rules.verdict_pos(buf, pos)[0]:
            return None
        return entryfunc_lengthfilter.__call__(self, buf, pos, globaloffset)


def _pushes_down_content(entryfunc):
    """... and its own content filter, unchanged, with rules of the unchanged class."""
    if not isinstance(entryfunc, entryfunc_contentfilter):
        return False
    t, r = type(entryfunc), type(entryfunc.rules)
    return ((t is entryfunc_contentfilter or (t.__call__ is entryfunc_contentfilter.__call__ and
                                              getattr(t, "keeps", None) is entryfunc_lengthfilter.keeps))
            and (r is ContentRules or (r.verdict is ContentRules.verdict and r.verdict_pos is ContentRules.verdict_pos)))


_M64 = (1 << 64) - 1


def _sm64(z):
    """the splitmix64 finaliser"""
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & _M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def seq_key(sequence):
    """The 64-bit key duplicate removal knows a read by (include/ffq.h states the rule at ffq_table_seq_keys; this is its host
    statement, in plain integers): a sum of one mixed term per four bytes of `sequence` -- little-endian, zero behind the
    end, the word's ordinal in the upper half --, mixed once more with the length; never 0.  Bytes are taken as they are."""
    s = bytes(sequence)
    n = len(s)
    total = 0
    for k in range((n + 3) // 4):
        total += _sm64(((k + 1) << 32) | int.from_bytes(s[4 * k:4 * k + 4], "little"))
    return _sm64((total + n * 0x9e3779b97f4a7c15) & _M64) or 1


def pair_key(k1, k2):
    """The key of a pair from its mates' keys, ordered; 0 (no key) if either mate has none."""
    if not k1 or not k2:
        return 0
    return _sm64((_sm64(k1) + k2) & _M64) or 1


class DedupRules:
    """Duplicate removal for filter_fastq / filter_fastq_paired (`fastp --dedup`; include/ffq.h states the rule): of the reads
    (pairs) the filters keep, those whose sequence -- as scanned, in front of any trim -- was seen before are dropped; the first
    copy in file order stays.  expected_reads: sizes the device set so that it need not grow (0: it grows as the file goes);
    max_bytes: cap of the device set (0: none); count_only: duplicates are counted (DedupReport), nothing is dropped."""

    def __init__(self, expected_reads=0, max_bytes=0, count_only=False):
        self.expected_reads, self.max_bytes, self.count_only = int(expected_reads), int(max_bytes), bool(count_only)
        if self.expected_reads < 0 or self.max_bytes < 0:
            raise ValueError("expected_reads and max_bytes are >= 0")


class DedupReport:
    """What filter_fastq(dedup_report=...) fills, of the reads (pairs) the filters kept: `keyed` had a key, `unkeyed` had none
    (wrapped records: always written), `distinct` different keys, `duplicates` = keyed - distinct."""

    def __init__(self):
        self.keyed = self.unkeyed = self.distinct = self.duplicates = 0

    @property
    def duplication_rate(self):
        return self.duplicates / self.keyed if self.keyed else 0.0

    def _from_counts(self, counts):
        """the six counts of a stream or a pair (hip: dedup_counts)"""
        self.keyed, self.unkeyed = counts[0] + counts[1] - counts[2], counts[2]
        self.duplicates, self.distinct = counts[1], counts[3]


class _HostDedup:
    """The set on the host route: a set of keys, and the DedupReport it counts into.  key(): of a record as scanned; keep(): is
    the record (of that key) written?"""

    def __init__(self, rules, report):
        self.drop, self.report, self.seen = not rules.count_only, report, set()

    @staticmethod
    def key(buf, pos):
        return seq_key(buf[pos[2]:pos[3]]) if adapter_trimmable(buf, pos) else 0

    def keep(self, key):
        rep = self.report
        if not key:
            rep.unkeyed += 1
            return True
        rep.keyed += 1
        if key in self.seen:
            rep.duplicates += 1
            return not self.drop
        self.seen.add(key)
        rep.distinct += 1
        return True


def _check_dedup(dedup, dedup_report):
    if dedup is not None and not isinstance(dedup, DedupRules):
        raise TypeError("dedup must be a DedupRules")
    if dedup_report is not None and dedup is None:
        raise ValueError("dedup_report needs dedup")
    if dedup_report is not None and not isinstance(dedup_report, DedupReport):
        raise TypeError("dedup_report must be a DedupReport")


class FilterReport:
    """What filter_fastq(report=...) fills: the statistics of the reads as they came in (`before`) and as they were written
    (`after`: behind the trims and the filters), and `dropped`: how many records each reason (ContentRules.REASONS) dropped."""

    def __init__(self, max_cycles=512):
        self.max_cycles = int(max_cycles)
        self.before = FastqStats(self.max_cycles)
        self.after = FastqStats(self.max_cycles)
        self.dropped = dict.fromkeys(ContentRules.REASONS, 0)


def _scanner(entrypos):
    """(the scanner, its open_stream or None): entrypos None is the GPU scanner, which has a native stream front end."""
    if entrypos is None:
        from . import _fastqandfurious as _C
        entrypos = _C.entrypos
    return entrypos, getattr(entrypos, 'open_stream', None)


def _configure_stream(st, trim, cutter, content, bounds, column=None, render=False, stats=None, dedup=None, poly_g=None, poly_x=None,
                      ends=None, umi=None):
    """What a native stream is asked for, in the order its chain works (csrc/ffq_stream.h states it above stream_chain): the UMI
    (umi: a UmiRules of a single file; taken in front of every trim, put into the names by the render), the
    ends (ends: (an EndRules, qual_base); fixed trims and sliding windows, in front of every other trim), the
    quality trim (an entryfunc_qualitytrim), the poly tails (poly_g / poly_x: a min_len each; one call for both steps, where
    the first of them works: poly-G runs in front of the adapter trim, poly-X behind it), the adapter trim (an
    entryfunc_adaptertrim), the content rules, the length
    filter (bounds: (min_len, max_len)) with the gathered column, the render, the statistics (stats: (qual_base,
    max_cycles)), the duplicate removal (dedup: a DedupRules; the stream takes the keys in front of the trims and asks its set
    behind the filter).  None / False: that setter is not called.  A stage that is added to the chain is added HERE."""
    if dedup is not None:
        st.set_dedup(not dedup.count_only, dedup.expected_reads, dedup.max_bytes)
    if umi is not None:
        st.set_umi(umi)
    if ends is not None:
        st.set_ends(ends[0], ends[1])
    if trim is not None:
        st.set_trim(trim.cutoff_back, trim.cutoff_front, trim.qual_base)
    if poly_g is not None or poly_x is not None:
        st.set_poly(poly_g, poly_x)
    if cutter is not None:
        st.set_adapter(cutter.adapter, cutter.err_permille, cutter.min_overlap)
    if content is not None:
        st.set_content(content)
    if bounds is not None:
        st.set_filter(bounds[0], bounds[1], column)
    if render:
        st.set_render()
    if stats is not None:
        st.set_stats(_hip.STATS_IN | _hip.STATS_OUT, stats[0], stats[1])


class CompressReport:
    """What filter_fastq(compress="bgzf", compress_report=...) fills, summed over every output it compresses: the bytes of
    text that went in, the bytes of the BGZF members that came out (the EOF markers not counted), the members, and those
    of them that are stored blocks (text that does not compress); `ratio` = bytes_in / bytes_out."""

    def __init__(self):
        self.bytes_in = self.bytes_out = self.members = self.members_stored = 0

    @property
    def ratio(self):
        return self.bytes_in / self.bytes_out if self.bytes_out else 0.0

    def _add_counts(self, stats):
        """(bytes in, bytes out, members, members stored) (hip: compressed, merged_bgzf)"""
        self.bytes_in += stats[0]
        self.bytes_out += stats[1]
        self.members += stats[2]
        self.members_stored += stats[3]


def _check_compress(compress, compress_report):
    if compress not in _hip.COMPRESS_MODES:
        raise ValueError("compress: %r is not one of %s" % (compress, sorted(_hip.COMPRESS_MODES, key=str)))
    if compress_report is not None and compress is None:
        raise ValueError("compress_report needs compress")
    if compress_report is not None and not isinstance(compress_report, CompressReport):
        raise TypeError("compress_report must be a CompressReport")
    return _report(compress_report, CompressReport)         # (the one to fill)


class _BgzfSink:
    """One output file written as BGZF.  The device route hands it whole members, a fill's or a round's at a time
    (members()); the host route hands it text (write()), which it cuts into bgzf.block members of BGZF_BLOCK_BYTES -- other
    bytes than the device's, the same text.  finish() writes what is left and, once, the EOF marker."""

    def __init__(self, fh, report):
        self.fh, self.report, self.buf = fh, report, bytearray()

    def members(self, members, stats):
        if stats[1]:
            self.fh.write(memoryview(members))
        self.report._add_counts(stats)

    def _block(self, chunk):
        from . import bgzf
        m = bgzf.block(chunk, 1)
        self.fh.write(m)
        self.report._add_counts((len(chunk), len(m), 1, int((m[18] & 6) == 0)))

    def write(self, text):
        self.buf += text
        size = _hip.BGZF_BLOCK_BYTES
        while len(self.buf) >= size:
            self._block(bytes(self.buf[:size]))
            del self.buf[:size]

    def finish(self):
        if self.buf:
            self._block(bytes(self.buf))
            self.buf = bytearray()
        self.fh.write(_hip.BGZF_EOF)


class _MateSettings:
    """What filter_fastq's one _MatePlan and filter_fastq_paired's two are built from beside each file's own arguments: the
    settings the mates share, with the three reports the plans ADD to checked -- poly, ends, compress: in this order -- and made
    (_report).  ends: the file's EndRules or, of a pair, one that is on for some mate; None: none is."""

    def __init__(self, quality_cutoff, qual_base, err_permille, min_overlap, content, poly_g, poly_x, poly_report, compress,
                 compress_report, ends, ends_report):
        self.quality_cutoff, self.qual_base, self.err_permille, self.min_overlap = quality_cutoff, qual_base, err_permille, min_overlap
        self.content, self.poly_g, self.poly_x, self.compress = content, poly_g, poly_x, compress
        if poly_report is not None and not isinstance(poly_report, PolyReport):
            raise TypeError("poly_report must be a PolyReport")
        self.poly_report = _report(poly_report, PolyReport)
        if _check_ends(ends) is None and ends_report is not None:
            raise ValueError("ends_report needs ends")
        if ends_report is not None and not isinstance(ends_report, EndsReport):
            raise TypeError("ends_report must be an EndsReport")
        self.ends_report = _report(ends_report, EndsReport)
        self.compress_report = _check_compress(compress, compress_report)


class _MatePlan:
    """What the records of ONE input file go through in filter_fastq (one plan) and filter_fastq_paired (one per mate), said
    once for both routes: the ends (an EndRules), quality trim, poly-G, adapter trim, poly-X, the verdict by length and then by
    content, the counts, the text.  shared: the _MateSettings of the call -- a pair's two plans ADD to one PolyReport, one
    EndsReport and one CompressReport; the rest is this file's own.  On the
    device route the plan configures the file's stream and drains every fill (or round) of it; on the host route it is
    called record by record.  judged=False: the mate is trimmed, counted and written but never dropped (pair_filter "first").
    `dropped`: this file's records by the reason (ContentRules.REASONS) they failed for; `report` (a FilterReport or None) is
    reset and bound to it.  compress ("bgzf" or None): the text is written as BGZF -- sink() wraps an output file for it,
    and everything that is written goes through what sink() returned."""

    def __init__(self, shared, adapter, min_len, max_len, report, judged=True, dedup=None, ends=None, umi=None, umi_report=None, mate=0):
        quality_cutoff, qual_base = shared.quality_cutoff, shared.qual_base
        # umi: the call's UmiRules (checked: _check_umi); mate 0: the one file of filter_fastq, 1 / 2: a pair's -- the PAIR sets the
        # rule on the device then (_PairPlan.configure), and this mate loses bases only if the location names it
        self.umi, self.umi_report, self.mate = umi, umi_report, mate
        self.umi_takes = umi is not None and (mate == 0 or umi.takes(mate))
        self.qual_base, self.content, self.report, self.judged = qual_base, shared.content, report, judged
        self.ends, self.ends_report = _check_ends(ends), shared.ends_report
        if ends is not None:
            _ends_qual_base(qual_base)
        self.compress, self.compress_report = shared.compress, shared.compress_report
        self.poly_g, self.poly_x = _poly_min_len("poly_g", shared.poly_g), _poly_min_len("poly_x", shared.poly_x)
        self.poly_report = shared.poly_report
        self.dedup = dedup           # (a single file's DedupRules; a pair's duplicates are the PairStream's, not a mate's)
        self.dropped = dict.fromkeys(ContentRules.REASONS, 0)
        if report is not None:
            report.dropped = self.dropped
            report.before = FastqStats(report.max_cycles, qual_base)
            report.after = FastqStats(report.max_cycles, qual_base)
        self.trim = self.cutter = None
        if quality_cutoff is not None:
            front, back = (0, quality_cutoff) if isinstance(quality_cutoff, (int, np.integer)) else quality_cutoff
            self.trim = entryfunc_qualitytrim(back, front, qual_base)            # (checks the ranges)
        if adapter is not None:
            self.cutter = entryfunc_adaptertrim(adapter, shared.err_permille, shared.min_overlap)    # (the adapter alone: the plan orders the trims)
        self.lo = None if min_len is None else int(min_len)
        self.hi = None if max_len is None else int(max_len)

    # ---- the device route
    def configure(self, st):
        """the file's stream: what is switched on, the render, and the statistics if there is a report"""
        rep = self.report
        _configure_stream(st, self.trim, self.cutter, self.content, None if self.lo is None and self.hi is None else (self.lo, self.hi),
                          render=True, stats=None if rep is None else (self.qual_base, rep.max_cycles), dedup=self.dedup,
                          poly_g=self.poly_g, poly_x=self.poly_x, ends=None if self.ends is None else (self.ends, self.qual_base),
                          umi=self.umi if self.mate == 0 else None)
        if self.compress is not None:
            st.set_compress(self.compress)

    def sink(self, fh_out):
        """what an output file is written through: itself, or with compress its BGZF writer"""
        return fh_out if self.compress is None or fh_out is None else _BgzfSink(fh_out, self.compress_report)

    def end(self, out):
        """behind the last write to what sink() returned: a compressed file gets its last member and the EOF marker"""
        if isinstance(out, _BgzfSink):
            out.finish()

    def drain(self, st, fh_out):
        """One fill (or round) of the stream: its text -- or, compressed, its members -- written with one write, its drops
        counted; (bytes of TEXT written, rows rendered, bases the trims removed)."""
        text, (nb, rendered, _skipped) = st.rendered()
        if self.compress is not None:
            fh_out.members(*st.compressed())
        elif nb:
            fh_out.write(memoryview(text))
        if st.filtered and self.judged:
            for reason, k in zip(ContentRules.REASONS, st.filter_counts()[1:7]):
                self.dropped[reason] += k
        removed = 0
        if self.umi is not None:
            u = st.umi_counts()
            removed += u[1]
            self.umi_report._add_counts(u)
        if self.ends is not None:
            e = st.ends_trimmed()
            removed += e[1]
            self.ends_report._add_counts(e)
        if self.trim is not None:
            removed += st.trimmed()[1]
        if self.cutter is not None:
            removed += st.adapter_trimmed()[1]
        if self.poly_g is not None or self.poly_x is not None:
            g, x = st.poly_trimmed()
            removed += g[1] + x[1]
            self.poly_report._add_counts((g, x))
        return nb, rendered, removed

    def finish(self, st):
        """the statistics the stream counted, read back once"""
        rep = self.report
        if rep is not None:
            rep.before = FastqStats.from_words(st.stats(_hip.STATS_IN), rep.max_cycles, self.qual_base)
            rep.after = FastqStats.from_words(st.stats(_hip.STATS_OUT), rep.max_cycles, self.qual_base)

    # ---- the host route
    def trimmed_pos(self, buf, pos):
        """(the positions as the trims leave them, bases cut, the UMI taken off it or None) of a record as read, which is
        counted into `before`.  The UMI goes on WITH the record: nothing behind this looks for it in the buffer again."""
        length = pos[3] - pos[2]
        if self.report is not None:
            self.report.before.add_pos(buf, pos)
        g = x = 0
        tag = None
        if self.umi_takes:                                   # (in front of every trim; `before` and the dedup key saw the read as read)
            pos, tag, skipped = _umi_pos(buf, list(pos), self.umi)
            self.umi_report._add_counts((int(tag is not None), length - (pos[3] - pos[2]), int(skipped), 0))
        if self.ends is not None:                            # (the chain's order: ends, quality, poly-G, adapter, poly-X)
            pos, e = _ends_pos(buf, list(pos), self.ends, self.qual_base)
            if e:
                self.ends_report._add_counts((1, e))
        if self.trim is not None:
            pos = self.trim.trimmed_pos(buf, pos)
        if self.poly_g is not None:
            pos, g = _poly_pos(buf, list(pos), b"G", self.poly_g)
        if self.cutter is not None:
            pos = self.cutter.trimmed_pos(buf, pos)
        if self.poly_x is not None:
            pos, x = _poly_pos(buf, list(pos), None, self.poly_x)
        if g or x:
            self.poly_report._add_counts(((int(g > 0), g), (int(x > 0), x)))
        return pos, length - (pos[3] - pos[2]), tag

    def verdict(self, buf, pos):
        """0, or the 1-based reason (counted into `dropped`) the record fails for, as the trims (and the overlap) left it:
        its length first, then the content rules."""
        v = 0
        if self.judged:
            length = pos[3] - pos[2]
            if (self.lo is not None and length < self.lo) or (self.hi is not None and length > self.hi):
                v = 1
            elif self.content is not None:
                v = self.content.verdict_pos(buf, pos)[0]
        if v:
            self.dropped[ContentRules.REASONS[v - 1]] += 1
        return v

    def text(self, buf, pos, tags=None):
        """a kept record as it is written, which is counted into `after`; tags: the UMI or UMIs that go into its name (None, or
        one of them None: the name stays as it is)"""
        if self.report is not None:
            self.report.after.add_pos(buf, pos)
        header = buf[(pos[0] + 1):pos[1]]
        if tags is not None and None not in tags:
            header = umi_name(bytes(header), tags, self.umi)
            self.umi_report.reads_tagged += 1
        return b"".join((b"@", header, b"\n", buf[pos[2]:pos[3]], b"\n+\n", buf[pos[4]:pos[5]], b"\n"))


def fastq_stats(fh: typing.BinaryIO, fbufsize: int = 1 << 24, qual_base: int = 33, max_cycles: int = 512,
                entrypos: typing.Optional[typing.Callable] = None, duplication: bool = False) -> FastqStats:
    """The statistics of every record of a FASTQ stream.  entrypos None (the GPU scanner): the stream front end scans
    every buffer fill and counts its table on the device (ffq_stream_set_stats); no row is looked at here and the totals
    are read once at the end.  Any other scanner: a loop over readfastq_iter with FastqStats.add_pos.  Malformed input
    raises what readfastq_iter raises.
    duplication: the reads are also looked up in a set of sequence keys (DedupRules(count_only=True): the stream's dedup on the
    device, a set of seq_key on the host) and the result's keyed, distinct, duplicates and duplication_rate are set."""
    out = FastqStats(max_cycles, qual_base)
    hd = _HostDedup(DedupRules(count_only=True), DedupReport()) if duplication else None

    def with_duplication(res, rep):
        res.keyed, res.distinct, res.duplicates, res.duplication_rate = rep.keyed, rep.distinct, rep.duplicates, rep.duplication_rate
        return res
    entrypos, open_stream = _scanner(entrypos)
    st = open_stream(fh, fbufsize) if open_stream is not None else None
    if st is not None:
        try:
            st.set_stats(_hip.STATS_IN, qual_base, max_cycles)
            if duplication:
                st.set_dedup(False)
            for _rows, _fill, _fill_offset, end_state, err_offset in st:
                if end_state != _END_OK and end_state != _END_REFILL:
                    _raise_for_end(end_state, err_offset)
            res = FastqStats.from_words(st.stats(_hip.STATS_IN), max_cycles, qual_base)
            if duplication:
                hd.report._from_counts(st.dedup_counts())
                with_duplication(res, hd.report)
            return res
        finally:
            st.close()

    def count(buf, pos, globaloffset=None):
        out.add_pos(buf, pos)
        if hd is not None:
            hd.keep(hd.key(buf, pos))

    for _ in readfastq_iter(fh, fbufsize, count, entrypos):
        pass
    return with_duplication(out, hd.report) if duplication else out


FilterResult = namedtuple('FilterResult', 'records_in records_out bases_removed bytes_out')


def filter_fastq(fh: typing.BinaryIO, fh_out: typing.BinaryIO, fbufsize: int = 1 << 24, quality_cutoff=None,
                 qual_base: int = 33, min_len=None, max_len=None, entrypos: typing.Optional[typing.Callable] = None,
                 adapter=None, err_permille: int = 100, min_overlap: int = 3, report=None, content=None, dedup=None,
                 dedup_report=None, poly_g=None, poly_x=None, poly_report=None, compress=None,
                 compress_report=None, ends=None, ends_report=None, umi=None, umi_report=None) -> FilterResult:
    """Trim, filter and WRITE a FASTQ stream: the file `cutadapt -q 20 -m 30` leaves behind, which is what the tables of
    positions of the reference's user guide are kept for in the end ("to avoid saving a FASTQ file after each filtering or
    read-trimming step", doc/user-guide.rst:196-204).  Every record of `fh` is quality-trimmed (quality_cutoff: an int --
    the 3' end -- or a (front, back) pair, as entryfunc_qualitytrim orders them after its first argument; None: no
    trimming), then cut at the 3' adapter (adapter: bytes, with err_permille and min_overlap as adapter_cut takes them --
    `cutadapt -q 20 -a AGATCGGAAGAGC --no-indels -m 30`; None: no adapter), dropped if its trimmed length lies outside
    [min_len, max_len], and written to `fh_out` as

        b"@" + header + b"\\n" + sequence + b"\\n+\\n" + quality + b"\\n"

    -- the slices of entryfunc, a bare '+' line; a wrapped record stays wrapped (and untrimmed: the rules do not apply to
    it).  Returns FilterResult(records_in, records_out, bases_removed -- by both trims, over every record, the dropped ones
    included --, bytes_out).

    entrypos None (the GPU scanner): the stream front end scans, trims, filters and renders every buffer fill on the device
    (ffq_stream_set_trim / _set_adapter / _set_filter / _set_render) and this loop does one fh_out.write(memoryview) per fill -- a plain
    file is read by the library itself, any other readable object chunk by chunk into pinned memory.  Any other scanner:
    a loop over readfastq_iter that writes the same bytes record by record.  Malformed input raises what readfastq_iter
    raises, behind the records in front of it; `fh` is left where that iterator leaves it.

    A read trimmed to length 0 is written as b"@h\\n\\n+\\n\\n" unless min_len >= 1 drops it.  A file with such records
    is read back record for record by the Python scanner (entrypos of this module) only: the GPU scanner answers as the
    reference's C scanner does and reads an empty record and the one behind it as one longer record, without an error.
    min_len >= 1 is what makes the output safe for the GPU scanner and for other tools.

    report: a FilterReport; its `before` is filled with the statistics of the records as read (qual_base as given here),
    its `after` with those of the records as written -- counted on the device beside the rest (ffq_stream_set_stats, no
    host wait per fill) and read once at the end, or record by record with another scanner.  None: nothing is counted.
    Its `dropped` says how many records each reason dropped ("length" and the content rules'), with or without `content`.

    content: a ContentRules; a record that its trimmed length keeps is dropped by the first of its rules that fails (`cutadapt
    --max-n --max-ee`, `fastp -n -e -q -u -y`): judged on the device with the GPU scanner (ffq_stream_set_content), by
    ContentRules.verdict_pos with any other.  Rows the rules do not apply to (wrapped records) go by their length alone.

    dedup: a DedupRules; of the records the filters keep, one whose sequence AS READ (in front of the trims: two copies that a
    quality trim cut differently are still one read) was met before in the file is not written -- on the device with the GPU
    scanner (ffq_stream_set_dedup: a set of 64-bit keys that lives there across the fills), with a set of seq_key on the host.
    records_out does not count the duplicates; report.dropped does not either: dedup_report (a DedupReport) has the numbers.
    A wrapped record has no key and is always written.

    poly_g / poly_x: None, or the min_len (2..65535; fastp's default is 10) of a homopolymer tail trim (poly_tail_cut): poly_g
    cuts a G tail -- what a two-colour instrument reads where the fragment has ended -- behind the quality trim and IN FRONT
    of the adapter trim, so that the adapter is still found with its G tail gone (`fastp --trim_poly_g`); poly_x cuts a tail
    of any one base behind the adapter trim (`--trim_poly_x`).  On the device with the GPU scanner (ffq_stream_set_poly).
    bases_removed includes what they cut; poly_report (a PolyReport) has the numbers, the same on either route.  Not done:
    wrapped records, 5' tails, per-base poly-X counts.

    ends: None, or an EndRules: fixed trims (`fastp -f / -t / -b`, `cutadapt -u / -l`) and sliding-window quality cutting of
    both ends (`fastp -5 / -r / -3`, Trimmomatic's SLIDINGWINDOW), IN FRONT of the quality trim and every other step -- fastp's
    order; ends_cut is the rule.  On the device with the GPU scanner (ffq_stream_set_ends).  bases_removed includes what it
    cut; ends_report (an EndsReport) has the numbers, the same on either route.  The rule has not been checked against
    fastp's or Trimmomatic's sources.  Not done: windows above 64, wrapped records, push-down through readfastq_iter,
    per-stage counts.

    compress: None, or "bgzf": `fh_out` (a binary file object, NOT a gzip.open one) is written as BGZF, what bgzip writes --
    gzip members of at most BGZF_BLOCK_BYTES of text each, which `zcat`, gzip.open and this package's own readers
    (automagic_open, hip.gunzip_fd, hip.bgzf_range, readfastq_iter_range) read, the last three member-parallel.  With the
    GPU scanner every fill's text is deflated on the device behind the render (ffq_stream_set_compress) and only the members
    come back, one fh_out.write per fill; with any other scanner the text is buffered and written as zlib level 1 members:
    other bytes, the same text.  The EOF marker is written once at the end.  bytes_out stays the bytes of TEXT; compress_report
    (a CompressReport) has the compressed size.  Not done: members aligned to records, a .gzi index, plain gzip.

    umi: None, or a UmiRules with loc "read1" (`fastp --umi --umi_loc read1 --umi_len 8`): the first `length` bases of every
    read are its unique molecular identifier; they (and `skip` bases behind them) are taken off the read IN FRONT of every
    trim and put into the name of the record as it is written, in front of the name's first blank (umi_take, umi_name).
    `before` and the dedup keys see the read as read -- two reads with the same sequence and different UMIs are no
    duplicates --, every trim, the filters and `after` see it without its UMI.  A read shorter than the UMI keeps its bases and
    its name; a wrapped record is left alone.  On the device with the GPU scanner (ffq_stream_set_umi).  bases_removed
    includes the UMI and the skipped bases; umi_report (a UmiReport) has the numbers, the same on either route.  The rule
    has not been checked against fastp's source.  Not done: UMIs in the index part of a header, push-down through
    readfastq_iter / readfastq_iter_range."""
    if content is not None and not isinstance(content, ContentRules):
        raise TypeError("content must be a ContentRules")
    _check_dedup(dedup, dedup_report)
    urep = _check_umi(umi, umi_report, single=True)
    shared = _MateSettings(quality_cutoff, qual_base, err_permille, min_overlap, content, poly_g, poly_x, poly_report, compress,
                           compress_report, ends, ends_report)
    plan = _MatePlan(shared, adapter, min_len, max_len, report, dedup=dedup, ends=ends, umi=umi, umi_report=urep)
    fh_out = plan.sink(fh_out)
    hd = _HostDedup(dedup, _report(dedup_report, DedupReport)) if dedup is not None else None
    entrypos, open_stream = _scanner(entrypos)
    n_in = n_out = removed = n_bytes = 0
    st = open_stream(fh, fbufsize) if open_stream is not None else None
    if st is not None:
        try:
            plan.configure(st)
            for rows, _fill, _fill_offset, end_state, err_offset in st:
                nb, rendered, cut = plan.drain(st, fh_out)
                n_in += st.selected()[1] if st.filtered else rows.shape[0]
                n_out += rendered
                n_bytes += nb
                removed += cut
                if end_state != _END_OK and end_state != _END_REFILL:
                    _raise_for_end(end_state, err_offset)
            plan.finish(st)
            plan.end(fh_out)
            if hd is not None:
                hd.report._from_counts(st.dedup_counts())
        finally:
            st.close()
        return FilterResult(n_in, n_out, removed, n_bytes)

    def record(buf, pos, globaloffset=None):
        key = hd.key(buf, pos) if hd is not None else 0
        pos, cut, tag = plan.trimmed_pos(buf, pos)
        if plan.verdict(buf, pos) or (hd is not None and not hd.keep(key)):
            return cut, None
        return cut, plan.text(buf, pos, None if umi is None else (tag,))

    for cut, text in readfastq_iter(fh, fbufsize, record, entrypos):
        n_in += 1
        removed += cut
        if text is not None:
            fh_out.write(text)
            n_out += 1
            n_bytes += len(text)
    plan.end(fh_out)
    return FilterResult(n_in, n_out, removed, n_bytes)


def pair_id(header):
    """What two mates of a pair have in common in their headers (include/ffq.h states the rule at ffq_table_pair_names; this
    is its host statement): `header` -- bytes, as entryfunc cuts them -- up to, not including, its first space (0x20) or tab
    (0x09), all of it if there is none; and if that has at least two bytes and ends in b"/1" or b"/2", without those two.
    This package's own rule, not cutadapt's (which also drops a bare trailing 1, 2 or 3)."""
    h = bytes(header)
    for i, b in enumerate(h):
        if b == 0x20 or b == 0x09:
            h = h[:i]
            break
    if len(h) >= 2 and h[-2:] in (b"/1", b"/2"):
        h = h[:-2]
    return h


class OverlapRules:
    """When the two mates of a pair count as overlapping (include/ffq.h, ffq_table_pair_overlap; fastp's defaults): at least
    min_overlap positions, of which at most max_diff, and at most diff_permille thousandths (integer division), differ."""

    MAX_LEN = _hip.OVERLAP_MAX_LEN

    def __init__(self, min_overlap=30, max_diff=5, diff_permille=200):
        if not 1 <= int(min_overlap) <= self.MAX_LEN:
            raise ValueError("min_overlap is 1..%d" % self.MAX_LEN)
        if not 0 <= int(max_diff) <= self.MAX_LEN:
            raise ValueError("max_diff is 0..%d" % self.MAX_LEN)
        if not 0 <= int(diff_permille) <= 1000:
            raise ValueError("diff_permille is 0..1000")
        self.min_overlap, self.max_diff, self.diff_permille = int(min_overlap), int(max_diff), int(diff_permille)


_BASE_CLASS = np.full(256, 4, dtype=np.int8)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    _BASE_CLASS[list(_pair)] = _i


def pair_overlap(seq1, seq2, rules):
    """The insert size of a pair from the overlap of its mates, or None if they do not overlap (include/ffq.h states the rule
    at ffq_table_pair_overlap; this is its host statement).  seq1 / seq2: bytes of the two sequence lines; rules: an
    OverlapRules.  With a = seq1 and rb = the reverse complement of seq2, the candidates o = 0, 1, ..., len(a) - min_overlap,
    then -1, -2, ..., -(len(rb) - min_overlap) place rb[0] at a[o]; the FIRST whose overlapping positions differ in at most
    min(max_diff, overlap * diff_permille // 1000) places gives insert = len(seq2) + o.  Bases match whatever their case;
    any other byte (N) matches nothing, not even itself.  insert < len(seq2) (o < 0) means the fragment is shorter than
    the reads: seq1[insert:] and seq2[insert:] are adapter."""
    n1, n2, mo = len(seq1), len(seq2), rules.min_overlap
    if n1 < mo or n2 < mo:
        return None
    a = _BASE_CLASS[np.frombuffer(seq1, dtype=np.uint8)]
    b = _BASE_CLASS[np.frombuffer(seq2, dtype=np.uint8)][::-1]
    rb = np.where(b < 4, 3 - b, 5)                    # (5: equal to no class of a, 4 included)
    for o in list(range(0, n1 - mo + 1)) + list(range(-1, -(n2 - mo) - 1, -1)):
        lo, hi = max(0, o), min(n1, n2 + o)
        mm = int(np.count_nonzero(a[lo:hi] != rb[lo - o:hi - o]))
        if mm <= min(rules.max_diff, (hi - lo) * rules.diff_permille // 1000):
            return n2 + o
    return None


def overlap_analysable(buf1, pos1, buf2, pos2):
    """Does the device analyse this pair (ffq_table_pair_overlap's eligibility)?  Both rows as adapter_trimmable asks, and
    neither mate above OverlapRules.MAX_LEN bases."""
    return (adapter_trimmable(buf1, pos1) and adapter_trimmable(buf2, pos2) and pos1[3] - pos1[2] <= OverlapRules.MAX_LEN
            and pos2[3] - pos2[2] <= OverlapRules.MAX_LEN)


class OverlapReport:
    """What filter_fastq_paired(overlap_report=...) fills: pairs_analysed, pairs_overlapped (an insert size was found),
    pairs_trimmed (at least one mate was cut), bases_removed = [from mate 1, from mate 2], insert_hist[i] = pairs with
    insert size i (uint64[hip.OVERLAP_HIST_WORDS]); insert_peak: the most frequent insert size (the smallest of several),
    None if no pair overlapped."""

    def __init__(self):
        self.pairs_analysed = self.pairs_overlapped = self.pairs_trimmed = 0
        self.bases_removed = [0, 0]
        self.insert_hist = np.zeros(_hip.OVERLAP_HIST_WORDS, dtype=np.uint64)

    def _add_counts(self, counts):
        """(pairs analysed, with an overlap, changed, bases removed from mate 1, from mate 2, ...) (hip: overlap)"""
        self.pairs_analysed += counts[0]
        self.pairs_overlapped += counts[1]
        self.pairs_trimmed += counts[2]
        self.bases_removed[0] += counts[3]
        self.bases_removed[1] += counts[4]

    @property
    def insert_peak(self):
        return int(np.argmax(self.insert_hist)) if self.insert_hist.any() else None


_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _x, _y in (b"AT", b"CG", b"at", b"cg"):
    _COMPLEMENT[_x], _COMPLEMENT[_y] = _y, _x


def merge_mates(seq1, qual1, seq2, qual2, insert):
    """The two mates of a pair merged into one read, or None if `insert` does not allow it (include/ffq.h states the rule at
    ffq_table_pair_merge; this is its host statement).  seq / qual: bytes of the four lines as they stand, behind any trim;
    insert: pair_overlap's.  With o = insert - len(seq2), position p of the merged read faces a[p] (p < n1) and byte
    bi = n2 - 1 - (p - o) of mate 2 (0 <= p - o < n2), read backwards and complemented; where both are there, mate 2's base and
    quality are taken if its quality byte is the higher one (unsigned; a tie goes to mate 1).  L = n2 + o for o < 0 (what lies
    beyond is adapter), else max(n1, n2 + o).  Returns (bases, quals), bytes of length L.  None: insert None or negative, a
    line pair of two lengths, a mate above OverlapRules.MAX_LEN, or not -n2 < o < n1."""
    n1, n2 = len(seq1), len(seq2)
    if insert is None or insert < 0 or len(qual1) != n1 or len(qual2) != n2 or n1 > OverlapRules.MAX_LEN or n2 > OverlapRules.MAX_LEN:
        return None
    o = int(insert) - n2
    if not -n2 < o < n1:
        return None
    L = n2 + o if o < 0 else max(n1, n2 + o)
    p = np.arange(L)
    in_a, in_b = p < n1, (p >= o) & (p < o + n2)
    a, qa, b, qb = (np.zeros(L, dtype=np.uint8) for _ in range(4))
    k = min(n1, L)
    a[:k] = np.frombuffer(seq1, dtype=np.uint8)[:k]
    qa[:k] = np.frombuffer(qual1, dtype=np.uint8)[:k]
    lo, hi = max(0, o), min(L, o + n2)
    b[lo:hi] = _COMPLEMENT[np.frombuffer(seq2, dtype=np.uint8)][::-1][lo - o:hi - o]
    qb[lo:hi] = np.frombuffer(qual2, dtype=np.uint8)[::-1][lo - o:hi - o]
    take_b = np.where(in_a & in_b, qb > qa, ~in_a)
    return np.where(take_b, b, a).tobytes(), np.where(take_b, qb, qa).tobytes()


def merge_mergeable(buf1, pos1, buf2, pos2, insert):
    """Does the device merge this pair (ffq_table_pair_merge's eligibility)?  Both rows' pos2..pos5 inside their buffers and in
    order with sequence and quality of one length, mate 1's header slice buf1[pos0 + 1:pos1] inside its buffer, neither mate
    above OverlapRules.MAX_LEN bases, insert >= 0 and -n2 < insert - n2 < n1.  Newlines are not looked for."""
    # (correct_correctable asks the rest: the correction does not look at the header)
    return bool(pos1[0] >= 0 and pos1[0] + 1 <= pos1[1] <= len(buf1)) and correct_correctable(buf1, pos1, buf2, pos2, insert)


class MergeReport:
    """What filter_fastq_paired(merge_report=...) fills: pairs_merged, bases_merged (bases of the merged reads), bytes_merged
    (bytes written to merged_out), overlap_positions (positions at which both mates had a base) and taken_from_mate2 (of
    those, positions whose base and quality came from mate 2)."""

    def __init__(self):
        self.pairs_merged = self.bases_merged = self.bytes_merged = self.overlap_positions = self.taken_from_mate2 = 0

    def _add_counts(self, counts):
        """(pairs merged, not merged, bytes of text, bases, positions inside overlaps, of those taken from mate 2) (hip: merged)"""
        self.pairs_merged += counts[0]
        self.bytes_merged += counts[2]
        self.bases_merged += counts[3]
        self.overlap_positions += counts[4]
        self.taken_from_mate2 += counts[5]


class CorrectionRules:
    """When a mismatched base inside the mates' overlap is corrected (include/ffq.h, ffq_table_pair_correct; fastp's values): the
    other mate's call has a quality of good_quality or more and this one's of bad_quality or less."""

    def __init__(self, good_quality=30, bad_quality=14):
        if not 0 <= int(bad_quality) < int(good_quality):
            raise ValueError("0 <= bad_quality < good_quality")
        if int(good_quality) > 255:
            raise ValueError("good_quality is at most 255 - qual_base")
        self.good_quality, self.bad_quality = int(good_quality), int(bad_quality)


class CorrectionReport:
    """What filter_fastq_paired(correction_report=...) fills: pairs_checked (pairs the rule looked at), pairs_corrected (at
    least one base was), bases_corrected = [in mate 1, in mate 2], mismatches (positions of the overlaps at which the mates
    disagree, corrected or not) and matrix[class before][class after] (int64[5][4]; classes A C G T, 4 = any other byte), both
    mates together."""

    def __init__(self):
        self.pairs_checked = self.pairs_corrected = self.mismatches = 0
        self.bases_corrected = [0, 0]
        self.matrix = np.zeros((5, 4), dtype=np.int64)

    def _add_counts(self, counts):
        """(pairs looked at, with a correction, bases corrected in mate 1, in mate 2, mismatch positions, ...) (hip: corrected)"""
        self.pairs_checked += counts[0]
        self.pairs_corrected += counts[1]
        self.bases_corrected[0] += counts[2]
        self.bases_corrected[1] += counts[3]
        self.mismatches += counts[4]


def _check_correction(rules, qual_base):
    if not isinstance(rules, CorrectionRules):
        raise TypeError("correction must be a CorrectionRules")
    if not (0 <= int(qual_base) and int(qual_base) + rules.good_quality <= 255):
        raise ValueError("qual_base + good_quality is at most 255")


def _correct_lines(seq1, qual1, seq2, qual2, insert, rules, qual_base):
    """correct_mates' work: None if the lines and `insert` do not let the pair be looked at, else (seq1, qual1, seq2, qual2,
    corrected in mate 1, in mate 2, mismatch positions, matrix int64[5][4])."""
    _check_correction(rules, qual_base)
    n1, n2 = len(seq1), len(seq2)
    if insert is None or insert < 0 or len(qual1) != n1 or len(qual2) != n2 or n1 > OverlapRules.MAX_LEN or n2 > OverlapRules.MAX_LEN:
        return None
    o = int(insert) - n2
    if not -n2 < o < n1:
        return None
    good, bad = qual_base + rules.good_quality, qual_base + rules.bad_quality
    a, qa, b, qb = (np.frombuffer(bytes(x), dtype=np.uint8).copy() for x in (seq1, qual1, seq2, qual2))
    p = np.arange(max(0, o), min(n1, n2 + o))
    bi = n2 - 1 - (p - o)
    ca, cb = _BASE_CLASS[a[p]], _BASE_CLASS[b[bi]]
    mismatch = ~((ca < 4) & (cb < 4) & (ca == 3 - cb))
    fix2 = mismatch & (qa[p] >= good) & (qb[bi] <= bad) & (ca < 4)
    fix1 = mismatch & ~fix2 & (qb[bi] >= good) & (qa[p] <= bad) & (cb < 4)
    matrix = np.zeros((5, 4), dtype=np.int64)
    np.add.at(matrix, (cb[fix2], 3 - ca[fix2]), 1)
    np.add.at(matrix, (ca[fix1], 3 - cb[fix1]), 1)
    # (positions are independent: every right-hand side is of the lines as they came)
    new_b, new_qb, new_a, new_qa = _COMPLEMENT[a[p[fix2]]], qa[p[fix2]], _COMPLEMENT[b[bi[fix1]]], qb[bi[fix1]]
    b[bi[fix2]], qb[bi[fix2]], a[p[fix1]], qa[p[fix1]] = new_b, new_qb, new_a, new_qa
    return (a.tobytes(), qa.tobytes(), b.tobytes(), qb.tobytes(), int(np.count_nonzero(fix1)), int(np.count_nonzero(fix2)),
            int(np.count_nonzero(mismatch)), matrix)


def correct_mates(seq1, qual1, seq2, qual2, insert, rules, qual_base=33):
    """Mismatched bases inside the overlap of a pair's mates corrected by the surer mate (include/ffq.h states the rule at
    ffq_table_pair_correct; this is its host statement).  seq / qual: bytes of the four lines as they stand, behind any trim;
    insert: pair_overlap's; rules: a CorrectionRules.  With o = insert - len(seq2), position p of mate 1 faces byte
    bi = n2 - 1 - (p - o) of mate 2; where the two do not match (by class, as pair_overlap matches: an N matches nothing) and
    one quality byte is >= qual_base + good_quality while the other is <= qual_base + bad_quality, the poor mate's base becomes
    the complement of the sure one -- if that is a base -- and its quality the sure one's.  Returns (seq1, qual1, seq2, qual2,
    bases corrected in mate 1, in mate 2); the lines unchanged and 0, 0 where the pair is not looked at (insert None or
    negative, a line pair of two lengths, a mate above OverlapRules.MAX_LEN, or not -n2 < o < n1)."""
    r = _correct_lines(seq1, qual1, seq2, qual2, insert, rules, qual_base)
    if r is None:
        return bytes(seq1), bytes(qual1), bytes(seq2), bytes(qual2), 0, 0
    return r[:6]


def correct_correctable(buf1, pos1, buf2, pos2, insert):
    """Does the device look at this pair (ffq_table_pair_correct's eligibility)?  merge_mergeable without its question about
    mate 1's header: both rows' pos2..pos5 inside their buffers and in order with sequence and quality of one length, neither
    mate above OverlapRules.MAX_LEN bases, insert >= 0 and -n2 < insert - n2 < n1.  Newlines are not looked for."""
    for buf, pos in ((buf1, pos1), (buf2, pos2)):
        p2, p3, p4, p5 = pos[2], pos[3], pos[4], pos[5]
        if not (p2 >= 0 and p4 >= 0 and p2 <= p3 <= len(buf) and p4 <= p5 <= len(buf) and p3 - p2 == p5 - p4
                and p3 - p2 <= OverlapRules.MAX_LEN):
            return False
    n1, n2 = pos1[3] - pos1[2], pos2[3] - pos2[2]
    return insert is not None and insert >= 0 and -n2 < insert - n2 < n1


PairedFilterResult = namedtuple('PairedFilterResult', 'pairs_in pairs_out bases_removed bytes_out1 bytes_out2 dropped')

_PAIR_FILTERS = ("any", "both", "first")


def _raise_for_pair_end(end_state, err_mate, err_offset, names=None):
    """The ValueError of a paired run: a mate's own malformed input, files of two lengths, records that are not mates."""
    if end_state == _hip.END_ERR_PAIR_COUNT:
        raise ValueError("mate %d: the file holds more records than mate %d's: its first unpaired record is at byte %d"
                         % (err_mate, 3 - err_mate, err_offset))
    if end_state == _hip.END_ERR_PAIR_NAMES:
        id1, id2 = names if names is not None else (b"?", b"?")
        raise ValueError("pair %d: the two records are not mates: %r and %r" % (err_offset, id1, id2))
    try:
        _raise_for_end(end_state, err_offset)
    except ValueError as e:
        raise ValueError("mate %d: %s" % (err_mate, e)) from None


class _HostRecord:
    """A record of the paired host route, kept until its mate is there: `at` (where it is in its file), `name` (its pair_id, or
    None), `cut` (bases the trims removed so far), `buf` and `pos` (its buffer and its six positions as the trims left them),
    `key` (its seq_key as scanned, 0: none), `tag` (the UMI taken off it, or None: it goes with the record, whatever becomes of
    its buffer and positions)."""
    __slots__ = ("at", "name", "cut", "buf", "pos", "key", "tag")

    def __init__(self, at, name, cut, buf, pos, key, tag=None):
        self.at, self.name, self.cut, self.buf, self.pos, self.key, self.tag = at, name, cut, buf, pos, key, tag

    def cut_to(self, c):
        """the record with sequence and quality cut to their first `c` bytes"""
        p = self.pos
        return _HostRecord(self.at, self.name, self.cut + p[3] - p[2] - c, self.buf, (p[0], p[1], p[2], p[2] + c, p[4], p[4] + c), self.key, self.tag)

    def patched(self, seq, qual):
        """the record in a buffer of its own -- itself cut out, with `seq` and `qual` in place of its two lines -- and its
        positions shifted to it"""
        p = self.pos
        lo, hi = p[0], max(p[1], p[3], p[5])
        own = bytearray(self.buf[lo:hi])
        own[p[2] - lo:p[3] - lo] = seq
        own[p[4] - lo:p[5] - lo] = qual
        return _HostRecord(self.at, self.name, self.cut, bytes(own), tuple(x - lo for x in p), self.key, self.tag)


def _per_mate(x):
    """a bound for both mates or a (mate 1, mate 2) pair of them -> the pair"""
    a, b = tuple(x) if isinstance(x, (tuple, list)) else (x, x)
    return (None if a is None else int(a), None if b is None else int(b))


def _ends_per_mate(ends):
    """one EndRules (or None) for both mates or a (mate 1, mate 2) pair of them -> the pair, checked"""
    if not isinstance(ends, (tuple, list)):
        return (_check_ends(ends),) * 2
    if len(ends) != 2:
        raise ValueError("ends is an EndRules for both mates or a pair of them")
    return (_check_ends(ends[0]), _check_ends(ends[1]))


def _step(it):
    """(record, None), (None, None) at the end, (None, error)"""
    try:
        return next(it), None
    except StopIteration:
        return None, None
    except ValueError as e:
        return None, e


def _check_pair_end(ps, end_state, err_mate, err_offset):
    """behind a round's drains: the ValueError of a round of `ps` that did not end well"""
    if end_state != _END_OK and end_state != _END_REFILL:
        names = tuple(pair_id(h) for h in ps.mismatch()) if end_state == _hip.END_ERR_PAIR_NAMES else None
        _raise_for_pair_end(end_state, err_mate, err_offset, names)


class _PairPlan:
    """What belongs to the PAIR in filter_fastq_paired, beside the two mates' _MatePlans and said once for both routes: the
    verdict of the pair (pair_filter) and its names (check_names), the overlap (an OverlapRules or None), the correction (a
    CorrectionRules or None, with qual_base), the duplicate pairs (a DedupRules or None), the merge (merging: is there a
    merged_out) and, merging, how the merged text is compressed.  The four reports are the caller's or private ones (_report):
    the plan always fills them.  `dropped`: the dropped pairs by the mate that failed.  On the device route the plan configures
    the hip.PairStream and drains every round of it; on the host route it is called pair by pair, with _HostRecords."""

    def __init__(self, pair_filter, check_names, overlap, overlap_report, correction, qual_base, correction_report, dedup, dedup_report,
                 merging, merge_report, compress, umi=None):
        self.umi = umi               # (the pair's UmiRules: set on the device by the pair; tags() says what a pair's names get)
        self.pair_filter, self.check_names, self.overlap, self.correction, self.qual_base = pair_filter, check_names, overlap, correction, qual_base
        self.dedup, self.merging, self.compress = dedup, merging, compress
        self.overlap_report, self.correction_report, self.merge_report = overlap_report, correction_report, merge_report
        self.hd = _HostDedup(dedup, dedup_report) if dedup is not None else None
        self.dropped = {"mate1_only": 0, "mate2_only": 0, "both": 0}

    # ---- the device route
    def configure(self, ps):
        """What the pair is asked for, in the order its round works: the overlap behind the mates' trims, the correction, the
        merge (with the compression of its text) and, between the filter and the merge, the duplicates.  None / False: that
        setter is not called.  A stage of the PAIR that is added is added HERE."""
        if self.umi is not None:
            ps.set_umi(self.umi)
        if self.overlap is not None:
            ps.set_overlap(self.overlap)
        if self.correction is not None:
            ps.set_correct(self.correction, self.qual_base)
        if self.merging:
            ps.set_merge()
            if self.compress is not None:
                ps.set_compress(self.compress)
        if self.dedup is not None:
            ps.set_dedup(not self.dedup.count_only, self.dedup.expected_reads, self.dedup.max_bytes)

    def drain(self, ps, merged_out):
        """One round of the pair: its merged text -- or, compressed, its members -- written with one write, the reports and
        `dropped` counted; (pairs merged: kept, and not among the round's n_out; bases the overlap removed).
        No host wait: the insert sizes and the matrix are read in finish()."""
        merged = removed = 0
        if self.merging:
            text, counts = ps.merged()
            if self.compress is not None:
                merged_out.members(*ps.merged_bgzf())
            elif counts[2]:
                merged_out.write(memoryview(text))
            self.merge_report._add_counts(counts)
            merged = counts[0]
        if self.overlap is not None:
            counts = ps.overlap(hist=False)[0]
            self.overlap_report._add_counts(counts)
            removed = counts[3] + counts[4]
        if self.correction is not None:
            self.correction_report._add_counts(ps.corrected()[0])
        _kept, _dropped, only1, only2, both = ps.selected()[1]
        if self.pair_filter != "both":            # (under "both" a pair with one failed mate is kept)
            self.dropped["mate1_only"] += only1
            self.dropped["mate2_only"] += only2
        self.dropped["both"] += both
        return merged, removed

    def finish(self, ps):
        """what the pair counted over all rounds, read back once"""
        if self.overlap is not None:
            self.overlap_report.insert_hist = ps.overlap()[1]
        if self.correction is not None:
            self.correction_report.matrix = ps.corrected()[1]
        if self.hd is not None:
            self.hd.report._from_counts(ps.dedup_counts())

    # ---- the host route
    def recorder(self, plan):
        """the entryfunc of one mate's readfastq_iter: the record as a _HostRecord, trimmed by the mate's plan"""
        def record(buf, pos, globaloffset=None):
            at = pos[0] + (globaloffset or 0)
            name = pair_id(buf[(pos[0] + 1):pos[1]]) if self.check_names else None
            key = self.hd.key(buf, pos) if self.hd is not None else 0
            pos, cut, tag = plan.trimmed_pos(buf, pos)
            return _HostRecord(at, name, cut, buf, tuple(pos[i] for i in range(6)), key, tag)
        return record

    def tags(self, r1, r2):
        """what the names of BOTH mates of a pair get: the UMI the location names, both for "per_read" (None: no UMIs)"""
        if self.umi is None:
            return None
        return (r1.tag, r2.tag) if self.umi.loc == "per_read" else (r1.tag,) if self.umi.loc == "read1" else (r2.tag,)

    def overlap_cut(self, r1, r2):
        """the two records with the overlap's cut applied and the pair's insert size (None: none), and the report filled"""
        (buf1, pos1), (buf2, pos2) = (r1.buf, r1.pos), (r2.buf, r2.pos)
        if self.overlap is None or not overlap_analysable(buf1, pos1, buf2, pos2):
            return r1, r2, None
        n1, n2 = pos1[3] - pos1[2], pos2[3] - pos2[2]
        insert = pair_overlap(buf1[pos1[2]:pos1[3]], buf2[pos2[2]:pos2[3]], self.overlap)
        if insert is not None:
            self.overlap_report.insert_hist[insert] += 1
        if insert is None or insert >= n2:              # (o >= 0: the fragment is not shorter than mate 2)
            self.overlap_report._add_counts((1, int(insert is not None), 0, 0, 0))
            return r1, r2, insert
        c1, c2 = min(n1, insert), min(n2, insert)
        self.overlap_report._add_counts((1, 1, 1, n1 - c1, n2 - c2))
        return r1.cut_to(c1), r2.cut_to(c2), insert

    def corrected(self, r1, r2, insert):
        """the two records with the correction applied, and the report filled: a mate with a corrected base continues as a
        private buffer (_HostRecord.patched); everything behind (verdict, text, merged_text) takes buffer and positions from the
        record and sees the corrected bytes"""
        (buf1, pos1), (buf2, pos2) = (r1.buf, r1.pos), (r2.buf, r2.pos)
        if self.correction is None or not correct_correctable(buf1, pos1, buf2, pos2, insert):
            return r1, r2
        seq1, qual1, seq2, qual2, c1, c2, mismatches, matrix = _correct_lines(
            buf1[pos1[2]:pos1[3]], buf1[pos1[4]:pos1[5]], buf2[pos2[2]:pos2[3]], buf2[pos2[4]:pos2[5]], insert, self.correction, self.qual_base)
        self.correction_report._add_counts((1, int(c1 + c2 > 0), c1, c2, mismatches))
        self.correction_report.matrix += matrix
        return r1.patched(seq1, qual1) if c1 else r1, r2.patched(seq2, qual2) if c2 else r2

    def drops(self, v1, v2):
        """is the pair dropped by its mates' verdicts?  Counted into `dropped`."""
        by = (v1 or v2) if self.pair_filter == "any" else (v1 and v2) if self.pair_filter == "both" else v1
        if by:
            self.dropped["both" if (v1 and v2) else "mate1_only" if v1 else "mate2_only"] += 1
        return bool(by)

    def merged_text(self, r1, r2, insert):
        """the pair as one record (None: it is not merged), and the report filled; behind the cut, with the insert size found
        in front of it: the rule takes o against the current length of mate 2, the text is the same either way"""
        (buf1, pos1), (buf2, pos2) = (r1.buf, r1.pos), (r2.buf, r2.pos)
        if not self.merging or not merge_mergeable(buf1, pos1, buf2, pos2, insert):
            return None
        bases, quals = merge_mates(buf1[pos1[2]:pos1[3]], buf1[pos1[4]:pos1[5]], buf2[pos2[2]:pos2[3]], buf2[pos2[4]:pos2[5]], insert)
        n1, n2 = pos1[3] - pos1[2], pos2[3] - pos2[2]
        o = insert - n2
        lo, hi = max(0, o), min(n1, n2 + o)
        text = b"".join((b"@", buf1[(pos1[0] + 1):pos1[1]], b"\n", bases, b"\n+\n", quals, b"\n"))
        qa = np.frombuffer(buf1[pos1[4]:pos1[5]], dtype=np.uint8)[lo:hi]
        qb = np.frombuffer(buf2[pos2[4]:pos2[5]], dtype=np.uint8)[::-1][lo - o:hi - o]
        self.merge_report._add_counts((1, 0, len(text), len(bases), hi - lo, int(np.count_nonzero(qb > qa))))
        return text


def filter_fastq_paired(fh1: typing.BinaryIO, fh2: typing.BinaryIO, fh_out1: typing.BinaryIO, fh_out2: typing.BinaryIO,
                        fbufsize: int = 1 << 24, quality_cutoff=None, qual_base: int = 33, min_len=None, max_len=None,
                        adapter=None, adapter2=None, err_permille: int = 100, min_overlap: int = 3, content=None,
                        pair_filter: str = "any", check_names: bool = True, report=None, report2=None,
                        entrypos: typing.Optional[typing.Callable] = None, overlap=None,
                        overlap_report=None, merged_out: typing.Optional[typing.BinaryIO] = None,
                        merge_report=None, dedup=None, dedup_report=None, poly_g=None, poly_x=None,
                        poly_report=None, compress=None, compress_report=None, correction=None,
                        correction_report=None, ends=None, ends_report=None, umi=None, umi_report=None) -> PairedFilterResult:
    """filter_fastq for paired-end files: the i-th records of `fh1` and `fh2` are mates, and a pair is written or dropped
    TOGETHER, so that `fh_out1` and `fh_out2` stay record for record in step (`cutadapt -q 20 -a ... -A ... -m 30:20
    --pair-filter=any -o out1 -p out2 in1 in2`).  Every record is trimmed as filter_fastq trims it -- quality_cutoff for both
    mates, `adapter` for mate 1 and `adapter2` for mate 2 (None: that mate is not adapter-trimmed) -- and judged on its own
    by its trimmed length (min_len / max_len: an int for both mates or a (mate 1, mate 2) pair) and by `content` (a
    ContentRules, both mates).  With v1 / v2 the two verdicts, the pair is dropped if

        pair_filter "any"    v1 or v2 fails (cutadapt's default)
        pair_filter "both"   both fail
        pair_filter "first"  v1 fails; mate 2 is not judged at all

    check_names: the two records must be mates by their names, pair_id(header 1) == pair_id(header 2).

    Returns PairedFilterResult(pairs_in, pairs_out, bases_removed -- both mates, every record --, bytes_out1, bytes_out2,
    dropped = {"mate1_only", "mate2_only", "both"}: the dropped pairs by which mate failed; with "first": all in
    "mate1_only").  report / report2: FilterReports per mate -- `before` every record of that file, `after` its records as
    written, `dropped` that mate's records by the reason they failed for, judged alone, whatever became of the pair (with
    "first", report2.dropped stays zero).

    entrypos None (the GPU scanner): two streams walked in lockstep on the device (hip.PairStream; include/ffq.h, ffq_pair),
    one write per mate and round.  Any other scanner: two readfastq_iter loops zipped record by record, from the same host
    functions as filter_fastq's.  Both routes write the same bytes and raise ValueError for

        a malformed mate         "mate 2: Incomplete entry at byte ..." (what readfastq_iter raises, with the mate in front)
        files of two lengths     naming the mate whose file holds more records
        records that are no mates    naming the pair's ordinal and the two ids

    each behind the pairs already written (the GPU route writes whole rounds: a round with a name error writes nothing).

    overlap: an OverlapRules; behind the per-mate trims and in front of the filters, the overlap of the two mates is looked
    for (pair_overlap) and, where the fragment is shorter than the reads, both mates are cut to it -- adapters go without
    being named (what fastp does to pairs by default).  The order is quality, adapter, overlap, filter; bases_removed then
    includes what the overlap cut.  Pairs the rule does not apply to (overlap_analysable: wrapped records, mates above 512
    bases) are left as they are.  overlap_report: an OverlapReport, filled on either route with the same numbers (its
    insert_peak: the library's insert size).  None: nothing of this is done.

    merged_out: a writable binary file (needs `overlap`); the order is then quality, adapter, overlap, filter, merge: a pair
    the filter keeps and whose insert size lets the mates be merged (merge_mergeable, merge_mates: `fastp --merge`) is written
    ONCE, to merged_out, as one read under mate 1's header, and to neither fh_out1 nor fh_out2.  pairs_out still counts every
    pair the filter kept; bytes_out1 / bytes_out2 and report.after / report2.after count what went to those two files.
    merge_report: a MergeReport (needs merged_out), filled on either route with the same numbers.

    dedup: a DedupRules; behind the filter and in front of the merge, a pair whose two sequences AS READ were met before as a
    pair (pair_key of the mates' seq_key: ordered) is dropped; the first copy stays.  pairs_out does not count the duplicates,
    `dropped` and the FilterReports do not know them: dedup_report (a DedupReport, in pairs) has the numbers.

    poly_g / poly_x: filter_fastq's, a min_len that applies to both mates; either step works per mate, in front of the overlap:
    the order is quality, poly-G, adapter, poly-X, overlap, filter, so the overlap and the merge see the rows as the per-mate
    trims left them (fastp runs its poly-X behind its overlap trim: a departure).  poly_report: a PolyReport, both mates added
    together.
    ends: filter_fastq's, one EndRules for both mates or a (mate 1, mate 2) pair of them (either may be None), as min_len is;
    the step works per mate in front of every other one: the order is ends, quality, poly-G, adapter, poly-X, overlap, filter,
    so the overlap and the merge see the reads as it left them.  ends_report: an EndsReport, both mates added together.
    correction: a CorrectionRules (needs `overlap`; `fastp --correction`); behind the overlap and in front of the filters, every
    position of a pair's overlap at which the mates disagree, one call sure and the other poor, has the poor base and quality
    replaced (correct_correctable, correct_mates).  The order is quality, poly-G, adapter, poly-X, overlap, correct, filter,
    dedup, merge: `before` and the dedup keys are of the records as read; the filters, `after`, the merge and everything
    written see the corrected bytes.  correction_report: a CorrectionReport (needs `correction`), filled on either route with
    the same numbers.
    Not done: interleaved input or output.
    compress / compress_report: filter_fastq's, over `fh_out1`, `fh_out2` and `merged_out`: each is written as a BGZF file of
    its own, each mate's text deflated by its stream and the merged text by the pair (ffq_pair_set_compress); the report sums
    over the three.
    umi / umi_report: filter_fastq's, with loc "read1", "read2" or "per_read": the mate or mates it names lose their UMI in
    front of every other step -- the names check still compares the headers as read --, and BOTH mates' names get the same
    insert (per_read: mate 1's UMI, b"_", mate 2's; a pair one of whose named mates is too short for a UMI gets none).  Not
    with merged_out (ValueError): a merged read's name is not tagged.  umi_report: both mates added together."""
    urep = _check_umi(umi, umi_report, single=False, merging=merged_out is not None)
    if content is not None and not isinstance(content, ContentRules):
        raise TypeError("content must be a ContentRules")
    if pair_filter not in _PAIR_FILTERS:
        raise ValueError('pair_filter is "any", "both" or "first"')
    if overlap is not None and not isinstance(overlap, OverlapRules):
        raise TypeError("overlap must be an OverlapRules")
    if overlap_report is not None and overlap is None:
        raise ValueError("overlap_report needs overlap")
    if merged_out is not None and overlap is None:
        raise ValueError("merged_out needs overlap")
    if merge_report is not None and merged_out is None:
        raise ValueError("merge_report needs merged_out")
    if correction is not None and overlap is None:
        raise ValueError("correction needs overlap")
    if correction_report is not None and correction is None:
        raise ValueError("correction_report needs correction")
    if correction is not None:
        _check_correction(correction, qual_base)
    crep = _report(correction_report, CorrectionReport)
    _check_dedup(dedup, dedup_report)
    drep, mrep, orep = _report(dedup_report, DedupReport), _report(merge_report, MergeReport), _report(overlap_report, OverlapReport)
    los, his, ends_pair = _per_mate(min_len), _per_mate(max_len), _ends_per_mate(ends)
    shared = _MateSettings(quality_cutoff, qual_base, err_permille, min_overlap, content, poly_g, poly_x, poly_report, compress,
                           compress_report, ends_pair[0] or ends_pair[1], ends_report)
    plans = tuple(_MatePlan(shared, a, lo, hi, rep, judged, ends=e, umi=umi, umi_report=urep, mate=k) for a, lo, hi, rep, judged, e, k
                  in zip((adapter, adapter2), los, his, (report, report2), (True, pair_filter != "first"), ends_pair, (1, 2)))
    pair = _PairPlan(pair_filter, check_names, overlap, orep, correction, qual_base, crep, dedup, drep, merged_out is not None, mrep,
                     compress, umi)
    entrypos, open_stream = _scanner(entrypos)
    pairs_in = pairs_out = removed = 0
    n_bytes = [0, 0]
    # (compress: all three outputs are BGZF, filter_fastq's way, and compress_report sums over them)
    outs = (plans[0].sink(fh_out1), plans[1].sink(fh_out2), plans[0].sink(merged_out))
    sts = []
    if open_stream is not None:
        for fh in (fh1, fh2):
            st = open_stream(fh, fbufsize)
            if st is None:
                break
            sts.append(st)
        if len(sts) != 2:
            for st in sts:
                st.close()
            sts = []
    if sts:
        ps = None
        try:
            for plan, st in zip(plans, sts):
                plan.configure(st)
            ps = _hip.PairStream(sts[0], sts[1], pair_filter, check_names)
            pair.configure(ps)
            for n_in, n_out, end_state, err_mate, err_offset in ps:
                merged, cut = pair.drain(ps, outs[2])
                pairs_in, pairs_out, removed = pairs_in + n_in, pairs_out + n_out + merged, removed + cut
                for k, (plan, st) in enumerate(zip(plans, sts)):
                    nb, _rendered, cut = plan.drain(st, outs[k])
                    n_bytes[k] += nb
                    removed += cut
                _check_pair_end(ps, end_state, err_mate, err_offset)
            for plan, st in zip(plans, sts):
                plan.finish(st)
            for out in outs:
                plans[0].end(out)
            pair.finish(ps)
        finally:
            if ps is not None:
                ps.close()
            for st in sts:
                st.close()
        return PairedFilterResult(pairs_in, pairs_out, removed, n_bytes[0], n_bytes[1], pair.dropped)

    its = [iter(readfastq_iter(fh, fbufsize, pair.recorder(plan), entrypos)) for plan, fh in zip(plans, (fh1, fh2))]
    while True:
        (r1, e1), (r2, e2) = _step(its[0]), _step(its[1])
        for k, e in ((1, e1), (2, e2)):
            if e is not None:
                raise ValueError("mate %d: %s" % (k, e)) from None
        if r1 is None and r2 is None:
            break
        if r1 is None or r2 is None:
            _raise_for_pair_end(_hip.END_ERR_PAIR_COUNT, 1 if r2 is None else 2, (r1 if r2 is None else r2).at)
        if check_names and r1.name != r2.name:
            _raise_for_pair_end(_hip.END_ERR_PAIR_NAMES, 0, pairs_in, (r1.name, r2.name))
        pairs_in += 1
        r1, r2, insert = pair.overlap_cut(r1, r2)
        r1, r2 = pair.corrected(r1, r2, insert)
        v1, v2 = plans[0].verdict(r1.buf, r1.pos), plans[1].verdict(r2.buf, r2.pos)
        removed += r1.cut + r2.cut
        if pair.drops(v1, v2) or (pair.hd is not None and not pair.hd.keep(pair_key(r1.key, r2.key))):
            continue
        pairs_out += 1
        text = pair.merged_text(r1, r2, insert)
        if text is not None:
            outs[2].write(text)
            continue
        tags = pair.tags(r1, r2)
        for k, r in enumerate((r1, r2)):
            text = plans[k].text(r.buf, r.pos, tags)
            outs[k].write(text)
            n_bytes[k] += len(text)
    for out in outs:
        plans[0].end(out)
    return PairedFilterResult(pairs_in, pairs_out, removed, n_bytes[0], n_bytes[1], pair.dropped)


class RangeEntries:
    """What readfastq_iter_range returns: an iterator over ONE rank's entries of a file that `world` ranks read
    together, with what the ranks agreed on -- `record_base` (global ordinal of this rank's first record: entry i of
    this iterator is record record_base + i of the file), `n_records` (this rank's), `total_records` (the file's),
    `bounds` (the byte ranges), `comm` (the step's figures: transport, halo source, repair rounds)."""

    def __init__(self, shard, entryfunc, batch_rows):
        self._sh, self._entryfunc, self._batch = shard, entryfunc, int(batch_rows)
        res = shard.out
        self.record_base, self.total_records = int(res.record_base), int(res.total_records)
        self.n_records = int(res.row_hi - res.row_lo)
        self.bounds = list(shard.bounds)
        self.comm = {"transport": shard.sh.transport(), "halo_source": "file" if res.halo_source else "ranks",
                     "rescan_rounds": int(res.rounds), "regathers": int(res.regathers), "allgather_ms": float(res.allgather_ms)}
        self._gen = self._entries()

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def close(self):
        self._gen.close()
        self._sh.close()         # (a generator that never started has no `finally` to run)

    def _filtered(self, view):
        """entryfunc_lengthfilter over this rank's records with the filter ON THE DEVICE (FileShard.select): one item per
        record -- None for a dropped one, the filter's component for a kept one (/root/reference/doc/user-guide.rst:153-180) --
        or, yield_dropped=False, the kept records' items alone.  Only the kept rows (and, from a resident range, their
        gathered component) cross the link; a dropped record costs the host one pointer in a list."""
        sh, flt = self._sh, self._entryfunc
        k, idx = sh.select(flt.min_len, flt.max_len)
        step = self._batch
        for i0 in range(0, self.n_records, step):                       # windows of ORIGINAL records
            i1 = min(i0 + step, self.n_records)
            ka, kb = int(np.searchsorted(idx, i0)), int(np.searchsorted(idx, i1))
            where = np.ascontiguousarray(idx[ka:kb] - i0)
            if kb == ka:
                yield from _kept_items(flt.yield_dropped, i1 - i0, where)
                continue
            rows = sh.kept_rows(ka, kb)
            a, b = int(rows[0, 0]), int(rows[-1, 5]) + 1
            col = off = None
            if flt.column != "entry":
                # (None: the range is not resident -- slabs; a view that grew --: the kept rows' slices out of the file)
                col, off = sh.kept_column(ka, kb, flt.column, rows) or _cut_column(view[a:b], rows, a, flt.column)
            yield from _kept_items(flt.yield_dropped, i1 - i0, where, col, off, view[a:b], rows, a)

    def _entries(self):
        import mmap
        sh, entryfunc = self._sh, self._entryfunc
        mm = None
        try:
            if self.n_records and hasattr(sh, "host_bytes"):
                # (a BGZF shard: the rank's inflated bytes are in host memory, sliced with stream offsets like a map of a plain file)
                from .sharded import _Shifted
                base, arr = sh.host_bytes()
                mm = view = _Shifted(arr, base)
            elif self.n_records:
                mm = mmap.mmap(sh.fd, 0, access=mmap.ACCESS_READ)       # (the page cache holds the range: it was just read)
                view = memoryview(mm)
            if self.n_records and _pushes_down(entryfunc):
                yield from self._filtered(view)
                return
            for i0 in range(0, self.n_records, self._batch):
                i1 = min(i0 + self._batch, self.n_records)
                rows = sh.rows(i0, i1)
                a, b = int(rows[0, 0]), int(rows[-1, 5]) + 1
                # entryfunc_phred: the qualities from the step's own decode -- or, over slabs (nothing resident), decoded on the
                # device batch by batch.  Any entryfunc sees the batch's bytes, positions relative to them, and `a` as the
                # globaloffset that makes them absolute file offsets (entryfunc_abspos, :186-195)
                quals = None
                if entryfunc is entryfunc_phred and (sh.decoded or sh.slab_bytes):
                    quals = partial(sh.quals, i0, i1, rows) if sh.decoded else partial(sh.quals_from_file, rows)
                for chunk in _table_entries(entryfunc, view[a:b], rows, a, quals):
                    yield from chunk
        finally:
            if mm is not None:
                try:
                    view.release()
                    mm.close()
                except BufferError:
                    pass                  # (an entry handed out still views the map: it goes with the last reference)
            sh.close()


def readfastq_iter_range(path, rank: int, world: int, entryfunc: typing.Callable = entryfunc, comm=None, ctx=None,
                         start: int = 0, end: typing.Optional[int] = None, batch_rows: int = 1 << 15,
                         tail_bytes: typing.Optional[int] = None, head_bytes: typing.Optional[int] = None,
                         bounds: typing.Optional[typing.Sequence[int]] = None,
                         slab_bytes: typing.Optional[int] = None, bgzf: typing.Optional[bool] = None,
                         exchange: typing.Optional[typing.Callable] = None) -> RangeEntries:
    """readfastq_iter for ONE FILE read by `world` ranks (one process per GPU): rank `rank` gets the entries whose '@'
    lies in its byte range [S_rank, S_rank+1) of the file, the same objects in the same order the reference's
    iterator (:198-279) yields for them -- the ranks' iterators concatenated ARE readfastq_iter over the whole file.

    Collective: every rank calls it (and reaches its first entry only when all have: the ranges are proven against
    each other in one step, ffq_shard_step_*).  Each rank reads its own range of the file (plus 1 MiB either side)
    into its GPU's memory -- nothing is handed from rank to rank but eight words each -- (a 100 GiB file over 8 GPUs:
    12.5 GiB each); a range that does not fit there -- or slab_bytes= / FFQ_SHARD_SLAB_BYTES -- goes through one device
    buffer slab after slab (sharded.FileShard), the entries are the same.  Errors of the stream (the iterator's three ValueErrors,
    :262, :269, :272) are raised on every rank alike, before any entry is yielded.

    comm: None (world 1; or torch.distributed's default group hands the communicator id round), 128 bytes of
    ffq_shard_unique_id, or a hip.ShardWorld (logical ranks as threads).  entryfunc_phred: the qualities are decoded
    on the device with the scan.  Returns a RangeEntries (iterate it; .record_base is the global ordinal).

    A BGZF file (bgzip's output; bgzf=None: recognised by its first member, True / False: said by the caller) is read by
    ranges too -- the one compressed format that can be: every rank inflates the members that begin in its share of the
    compressed file, the entries are those of the UNCOMPRESSED stream, what readfastq_iter(gzip.open(path), ...) yields
    (sharded.BgzfFileShard; exchange: how the ranks tell each other their sizes when comm is not a transport object and
    torch.distributed is not there).  start / end / bounds / slab_bytes do not apply to it."""
    from . import hip as _hip, sharded as _sharded
    if ctx is None:
        ctx = _hip.default_context()
    if bgzf is None:
        bgzf = _sharded.is_bgzf(path)
        if not bgzf and _sharded.is_gzip(path):
            raise ValueError("readfastq_iter_range: %r is a gzip file but not BGZF -- ordinary gzip members cannot be entered in the "
                             "middle, so the file cannot be read by ranges; readfastq_iter(automagic_open(path), ...) streams it "
                             "(or recompress it with bgzip)" % (path,))
    if bgzf:
        if start or end is not None or bounds is not None or slab_bytes:
            raise ValueError("readfastq_iter_range: start / end / bounds / slab_bytes do not apply to a BGZF file")
        kwz = {}
        if tail_bytes is not None:
            kwz["tail_bytes"] = tail_bytes
        if head_bytes is not None:
            kwz["head_bytes"] = head_bytes
        sh = _sharded.BgzfFileShard(ctx, path, rank, world, comm=comm, exchange=exchange, **kwz)
        try:
            sh.load()
            sh.scan(decode=entryfunc is entryfunc_phred)
        except BaseException:
            sh.close()
            raise
        return RangeEntries(sh, entryfunc, batch_rows)
    kw = {}
    if tail_bytes is not None:
        kw["tail_bytes"] = tail_bytes
    if head_bytes is not None:
        kw["head_bytes"] = head_bytes
    if slab_bytes:
        kw["slab_bytes"] = slab_bytes
    sh = _sharded.FileShard(ctx, path, rank, world, comm=comm, start=start, end=end, bounds=bounds, **kw)
    try:
        sh.load()
        sh.scan(decode=entryfunc is entryfunc_phred and not sh.slab_bytes)      # (over slabs: decoded batch by batch, FileShard.quals_from_file)
    except BaseException:
        sh.close()
        raise
    return RangeEntries(sh, entryfunc, batch_rows)


# extension -> (module name or namespace, opener name, positional arguments after the file name)
FORMAT_OPENERS: typing.Dict[str, typing.Tuple[typing.Union[str, object], str, list]] = {
    'gz': ('gzip', 'open', list()),
    'gzip': ('gzip', 'open', list()),
    'bgz': ('gzip', 'open', list()),        # (bgzip's output is a gzip file: members that carry their length)
    'bz2': ('bz2', 'open', list()),
    'lzma': ('lzma', 'open', list()),
    'xz': ('lzma', 'open', list()),
}


def automagic_open(filename, openers=None) -> typing.BinaryIO:
    """Open a (presumably FASTQ) file, compressed or not, by its extension (reference
    :290-334): `foo/bar.fq.gz` through gzip, `foo/bar.fq` as a plain binary file.  `openers`
    maps extensions to (module name or namespace, function name, extra positional arguments);
    None means FORMAT_OPENERS.  The stream it returns feeds readfastq_iter: decompression
    runs on the host, the scan of every buffer fill on the GPU."""
    if openers is None:
        openers = FORMAT_OPENERS
    parts = str(filename).rsplit(os.path.extsep, maxsplit=1)
    ext = parts[-1] if len(parts) > 1 else None
    try:
        modulename, funcname, args = openers[ext]
    except KeyError:
        modulename, funcname, args = ('io', 'open', ('rb', ))
    module = importlib.import_module(modulename) if isinstance(modulename, str) else modulename
    return getattr(module, funcname)(filename, *args)
