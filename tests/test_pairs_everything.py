"""filter_fastq_paired with EVERY stage and every report switched on at once, the device route against the host route: ends,
quality trim, poly-G, adapters, poly-X, overlap, correction, content rules, min_len, dedup, merge -- plain and as BGZF.  The
three files (inflated where compressed), the result and every report are the same on both routes.  One input shows every
stage: the pairs of tests/correct_expect.py with G tails behind every second adapter, a T tail on some long fragments' mate 1
and every fifth pair a copy of the one in front of it.  What the host route makes of each stage is held against the rules'
loops by that stage's own tests (test_*_host.py, test_*_plan.py); here it is the reference."""
import functools
import gzip
import io

import numpy as np
import pytest

import correct_expect as K
import pairs_expect as P

N_PAIRS = 1500
FBUFS = (1 << 14, 3 << 13)
EOF_BYTES = 28


@pytest.fixture(scope="module")
def F(pkg):
    from fastqandfurious_amd import fastqandfurious
    return fastqandfurious


@pytest.fixture(scope="module")
def C(gpu_ctx):
    from fastqandfurious_amd import _fastqandfurious
    return _fastqandfurious


@functools.lru_cache(maxsize=None)
def files():
    r1, r2 = K.records(N_PAIRS)
    out = ([], [])
    for i in range(N_PAIRS):
        pair = []
        for (h, s, q), ad in ((r1[i], P.ADAPTER1), (r2[i], P.ADAPTER2)):
            p = s.find(ad)
            if 10 not in s:
                if p >= 0 and i % 2 and len(s) - p - len(ad) >= 10:        # the instrument ran past the fragment
                    s = s[:p + len(ad)] + b"G" * (len(s) - p - len(ad))
                elif p < 0 and i % 7 == 3 and ad == P.ADAPTER1:
                    s = s[:-15] + b"T" * 15
            pair.append((h, s, q))
        if i % 5 == 4:                                                     # a copy of the pair in front, under its own names
            pair = [(h, s, q) for (h, _s, _q), (_h, s, q) in zip(pair, (out[0][-1], out[1][-1]))]
        out[0].append(pair[0])
        out[1].append(pair[1])
    return K.file_of(out[0]), K.file_of(out[1])


def run(F, entrypos, fbufsize, compress):
    d1, d2 = files()
    outs = (io.BytesIO(), io.BytesIO(), io.BytesIO())
    reps = dict(report=F.FilterReport(), report2=F.FilterReport(), overlap_report=F.OverlapReport(), merge_report=F.MergeReport(),
                correction_report=F.CorrectionReport(), dedup_report=F.DedupReport(), poly_report=F.PolyReport(),
                ends_report=F.EndsReport())
    if compress:
        reps["compress_report"] = F.CompressReport()
    res = F.filter_fastq_paired(io.BytesIO(d1), io.BytesIO(d2), outs[0], outs[1], fbufsize, entrypos=entrypos, merged_out=outs[2],
                                ends=(F.EndRules(trim_front=1, right=(4, 15)), F.EndRules(trim_tail=1, front=(4, 15))),
                                quality_cutoff=(5, 15), poly_g=10, adapter=P.ADAPTER1, adapter2=P.ADAPTER2, poly_x=10,
                                overlap=F.OverlapRules(), correction=F.CorrectionRules(K.GOOD, K.BAD),
                                content=F.ContentRules(max_n=0, min_mean_quality=30), min_len=(40, 40), dedup=F.DedupRules(),
                                compress="bgzf" if compress else None, **reps)
    raw = tuple(o.getvalue() for o in outs)
    texts = tuple(gzip.decompress(x) for x in raw) if compress else raw
    said = {}
    for name, rep in reps.items():
        if name in ("report", "report2"):
            said[name] = (dict(rep.dropped), rep.before.words.tolist(), rep.after.words.tolist())
        elif name == "compress_report":
            # (the host route cuts the whole text into members, the device every round's: other members, the same text)
            assert rep.bytes_out == sum(len(x) for x in raw) - 3 * EOF_BYTES and rep.members >= 3
            said[name] = rep.bytes_in
        else:
            said[name] = {k: np.asarray(v).tolist() for k, v in vars(rep).items()}
    return tuple(res), texts, said


HOST = {}


def host(F, compress):
    """the host route's answer, computed once"""
    if compress not in HOST:
        HOST[compress] = run(F, F.entrypos, 1 << 14, compress)
    return HOST[compress]


def check_every_stage_shows(res, texts, said):
    """the leading count of each report, and then some: no stage is idle on this input"""
    assert said["ends_report"]["reads_cut"] > 100 and said["ends_report"]["bases_cut"] > 0
    poly = said["poly_report"]
    assert poly["poly_g_reads"] > 20 and poly["poly_x_reads"] > 20
    assert said["overlap_report"]["pairs_analysed"] > 1000 and said["overlap_report"]["pairs_trimmed"] > 50
    assert sum(said["overlap_report"]["insert_hist"]) == said["overlap_report"]["pairs_overlapped"] > 100
    corr = said["correction_report"]
    assert corr["pairs_checked"] > 100 and corr["pairs_corrected"] > 20 and min(corr["bases_corrected"]) > 0
    assert sum(sum(row) for row in corr["matrix"]) == sum(corr["bases_corrected"])
    assert said["merge_report"]["pairs_merged"] > 50 and said["merge_report"]["bytes_merged"] == len(texts[2])
    dedup = said["dedup_report"]
    assert dedup["keyed"] > 100 and dedup["duplicates"] > 50 and dedup["unkeyed"] > 0
    for name in ("report", "report2"):
        dropped = said[name][0]
        assert dropped["length"] > 0 and dropped["n"] > 0 and dropped["mean_quality"] > 0
    assert sum(res[5].values()) > 100 and all(res[5].values())
    # quality trim and adapters: more is removed than ends, poly tails and overlap account for
    assert res[2] > said["ends_report"]["bases_cut"] + poly["poly_g_bases"] + poly["poly_x_bases"] + sum(said["overlap_report"]["bases_removed"])
    assert res[0] == N_PAIRS and 0 < res[1] < N_PAIRS - dedup["duplicates"] and all(len(t) > 0 for t in texts)
    assert (res[3], res[4]) == (len(texts[0]), len(texts[1]))
    if "compress_report" in said:
        assert said["compress_report"] == sum(len(t) for t in texts)


@pytest.mark.parametrize("compress", (False, True), ids=("plain", "bgzf"))
def test_the_host_route_shows_every_stage(F, compress):
    check_every_stage_shows(*host(F, compress))
    assert host(F, True)[:2] == host(F, False)[:2]


@pytest.mark.gpu
def test_every_stage_and_report_device_against_host(F, C):
    for compress in (False, True):
        want = host(F, compress)
        check_every_stage_shows(*want)
        for fbufsize in FBUFS:
            assert len(files()[0]) > 10 * fbufsize                 # several rounds
            res, texts, said = run(F, C.entrypos, fbufsize, compress)
            assert texts == want[1]
            assert res == want[0]
            assert sorted(said) == sorted(want[2])
            for name in said:
                assert said[name] == want[2][name], name
