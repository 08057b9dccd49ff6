"""What the plan tests share (tests/test_filter_plan.py, test_poly_plan.py, test_plan_rounds.py, test_plan_errors.py): recording
fakes with the surface of hip._Stream and hip.PairStream, and a scanner whose open_stream hands them out.  No GPU, no library.
A fake logs every setter call with its arguments as the real signature binds them.  By default it yields no fill (no round);
with a script -- one dict per fill or round, keyed by the getter's name -- it yields the script's and every getter answers with
the entry of the fill (round) the iteration has just yielded."""
import io

import numpy as np
import pytest

ZEROS3 = (0, 0, 0)


class FakeStream:
    """hip._Stream's surface: every setter call is logged with its arguments as the real signature binds them."""
    decode = False

    def __init__(self, fail=None, script=()):
        self.log, self.fail, self.filtered, self.closed, self.cycles = [], fail, False, 0, 1
        self.script, self.at = list(script), -1

    def _call(self, name, *args):
        if name == self.fail:
            raise RuntimeError("%s refused" % name)
        self.log.append((name,) + args)

    def _now(self, name, default):
        return self.script[self.at].get(name, default) if self.at >= 0 else default

    def set_filter(self, min_seq_len=None, max_seq_len=None, column=None, value_add=0):
        self._call("set_filter", min_seq_len, max_seq_len, column, value_add)
        self.filtered = True

    def set_content(self, rules):
        self._call("set_content", rules)
        self.filtered = True

    def set_dedup(self, drop=True, expected_keys=0, max_bytes=0):
        self._call("set_dedup", drop, expected_keys, max_bytes)
        self.filtered = True

    def set_trim(self, cutoff_back, cutoff_front=0, qual_base=33):
        self._call("set_trim", cutoff_back, cutoff_front, qual_base)

    def set_adapter(self, adapter, err_permille=100, min_overlap=3):
        self._call("set_adapter", adapter, err_permille, min_overlap)

    def set_ends(self, rules, qual_base=33):
        self._call("set_ends", rules, qual_base)

    def set_poly(self, poly_g=None, poly_x=None):
        self._call("set_poly", poly_g, poly_x)

    def set_stats(self, which, qual_base=33, max_cycles=512):
        self._call("set_stats", which, qual_base, max_cycles)
        self.cycles = max_cycles

    def set_render(self):
        self._call("set_render")

    def set_compress(self, mode="bgzf"):
        self._call("set_compress", mode)

    # what a fill is asked for; without a script the fake yields none, so only stats() and dedup_counts() are ever reached
    def rendered(self):
        return self._now("rendered", (np.zeros(0, dtype=np.uint8), ZEROS3))

    def compressed(self):
        return self._now("compressed", (np.zeros(0, dtype=np.uint8), (0, 0, 0, 0)))

    def filter_counts(self):
        return self._now("filter_counts", [0] * 8)

    def trimmed(self):
        return self._now("trimmed", ZEROS3)

    def adapter_trimmed(self):
        return self._now("adapter_trimmed", ZEROS3)

    def ends_trimmed(self):
        return self._now("ends_trimmed", ZEROS3)

    def poly_trimmed(self):
        return self._now("poly_trimmed", (ZEROS3, ZEROS3))

    def selected(self):
        return self._now("selected", (np.zeros(0, dtype=np.int64), 0, None, None))

    def dedup_counts(self):
        return self._now("dedup_counts", [0] * 6)

    def stats(self, which):
        from fastqandfurious_amd import hip
        return np.zeros(hip.stats_words(self.cycles), dtype=np.uint64)

    def __iter__(self):
        """a fill of the script: its "next" = (rows, fill, fill_offset, end_state, err_offset)"""
        for self.at in range(len(self.script)):
            yield self.script[self.at]["next"]

    def close(self):
        self.closed += 1


class FakeScanner:
    """An `entrypos` with an open_stream attribute; fail: (ordinal of the stream, setter that raises); none_at: the ordinal
    at which open_stream declines (returns None, as the real one does for a source it cannot stream); scripts: one script
    per stream, in the order they are opened."""

    def __init__(self, fail=None, none_at=None, scripts=()):
        self.streams, self.fail, self.none_at, self.scripts = [], fail, none_at, scripts

    def open_stream(self, fh, fbufsize, decode=False):
        k = len(self.streams)
        if k == self.none_at:
            return None
        self.streams.append(FakeStream(self.fail[1] if self.fail is not None and self.fail[0] == k else None,
                                       self.scripts[k] if k < len(self.scripts) else ()))
        return self.streams[-1]

    def __call__(self, buf, offset, posbuffer):
        raise AssertionError("the host route was taken")


class NoRounds:
    """hip.PairStream's surface, yielding no round -- or the rounds of `script` (a class attribute, set by the test in front
    of the call: the filter makes the object), each with "next" = (n_in, n_out, end_state, err_mate, err_offset).  A round moves
    both mates' fakes to their entry of it.  `fail`: the setter that raises."""
    made = []
    script = ()
    fail = None

    def __init__(self, mate1, mate2, pair_filter="any", check_names=True):
        self.mates, self.closed, self.log, self.at = (mate1, mate2), 0, [], -1
        self.opened = (pair_filter, check_names)
        NoRounds.made.append(self)

    def _call(self, name, *args):
        if name == self.fail:
            raise RuntimeError("%s refused" % name)
        self.log.append((name,) + args)

    def _now(self, name, default):
        return self.script[self.at].get(name, default) if self.at >= 0 else default

    def set_overlap(self, rules, trim=True):
        self._call("set_overlap", rules, trim)

    def set_correct(self, rules, qual_base=33):
        self._call("set_correct", rules, qual_base)

    def set_merge(self, on=True):
        self._call("set_merge", on)

    def set_compress(self, mode="bgzf"):
        self._call("set_compress", mode)

    def set_dedup(self, drop=True, expected_keys=0, max_bytes=0):
        self._call("set_dedup", drop, expected_keys, max_bytes)

    def overlap(self, hist=True):
        from fastqandfurious_amd import hip
        counts, h = self._now("overlap", ([0] * 6, np.zeros(hip.OVERLAP_HIST_WORDS, dtype=np.uint64)))
        return counts, h if hist else None

    def corrected(self):
        return self._now("corrected", ([0] * 6, np.zeros((5, 4), dtype=np.int64)))

    def merged(self):
        return self._now("merged", (np.zeros(0, dtype=np.uint8), [0] * 6))

    def merged_bgzf(self):
        return self._now("merged_bgzf", (np.zeros(0, dtype=np.uint8), (0, 0, 0, 0)))

    def selected(self):
        return self._now("selected", (np.zeros(0, dtype=np.int64), [0] * 5))

    def dedup_counts(self):
        return self._now("dedup_counts", [0] * 6)

    def mismatch(self):
        return self._now("mismatch", (b"?", b"?"))

    def __iter__(self):
        for self.at in range(len(self.script)):
            for st in self.mates:
                st.at = self.at
            yield self.script[self.at]["next"]

    def close(self):
        self.closed += 1


@pytest.fixture
def no_rounds(monkeypatch):
    """hip.PairStream replaced by NoRounds for one test: NoRounds.made lists what the filter made"""
    from fastqandfurious_amd import hip
    NoRounds.made = []
    monkeypatch.setattr(hip, "PairStream", NoRounds)
    monkeypatch.setattr(NoRounds, "script", ())
    monkeypatch.setattr(NoRounds, "fail", None)
    return NoRounds


def single(F, scanner, **kw):
    return F.filter_fastq(io.BytesIO(b""), io.BytesIO(), 4096, entrypos=scanner, **kw)


def paired(F, scanner, **kw):
    return F.filter_fastq_paired(io.BytesIO(b""), io.BytesIO(b""), io.BytesIO(), io.BytesIO(), 4096, entrypos=scanner, **kw)
