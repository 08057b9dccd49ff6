"""The generated pairs of tools/bench_overlap.py and tools/bench_merge.py: a fragment of seeded length is read READ bases from
either end, mate 2 as the reverse complement; where the fragment is shorter than the read the adapters' bytes follow it; every
base is changed with probability `err`.  Records have one fixed size (REC bytes), so a table over them is written down, not
scanned."""
import numpy as np

READ = 150
ADAPTER1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA" * 5
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT" * 5
HEAD = 15                                         # b"@P%010d/1\n"
REC = HEAD + READ + 3 + READ + 1                  # bytes of a record
COMP = np.zeros(256, dtype=np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def pair_block(n_pairs, short, err, seed, qual=None):
    """(records of mate 1, records of mate 2) as uint8[n_pairs][REC], share of pairs with a fragment shorter than the read.
    qual None: every quality is b"I"; (lo, hi): seeded bytes in [lo, hi)"""
    rng = np.random.default_rng(seed)
    out = [np.empty((n_pairs, REC), dtype=np.uint8) for _ in (0, 1)]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    ad = [np.frombuffer(a, dtype=np.uint8)[:READ + 1] for a in (ADAPTER1, ADAPTER2)]
    j = np.arange(READ)[None, :]
    n_short = 0
    for lo in range(0, n_pairs, 1 << 17):
        k = min(1 << 17, n_pairs - lo)
        is_short = rng.random(k) < short
        n_short += int(is_short.sum())
        L = np.where(is_short, rng.integers(35, READ, k), rng.integers(300, 501, k))[:, None]
        f1 = bases[rng.integers(0, 4, (k, READ))]
        tail = np.clip(j - L, 0, READ)                            # place in the adapter behind a short fragment
        m1 = np.where(j < L, f1, ad[0][tail])
        back = np.take_along_axis(f1, np.clip(L - 1 - j, 0, READ - 1), axis=1)
        m2 = np.where(is_short[:, None], np.where(j < L, COMP[back], ad[1][tail]), bases[rng.integers(0, 4, (k, READ))])
        for k_mate, m in enumerate((m1, m2)):
            flip = rng.random((k, READ)) < err
            m = np.where(flip, bases[(np.searchsorted(bases, m) + rng.integers(1, 4, (k, READ))) % 4], m)
            rec = out[k_mate][lo:lo + k]
            num = np.arange(lo, lo + k)
            rec[:, 0], rec[:, 1] = ord("@"), ord("P")
            for d in range(10):
                rec[:, 2 + d] = 48 + (num // 10 ** (9 - d)) % 10
            rec[:, 12], rec[:, 13], rec[:, 14] = ord("/"), ord("1") + k_mate, 10
            rec[:, HEAD:HEAD + READ] = m
            rec[:, HEAD + READ:HEAD + READ + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, HEAD + READ + 3:REC - 1] = ord("I") if qual is None else rng.integers(qual[0], qual[1], (k, READ))
            rec[:, REC - 1] = 10
    return out[0], out[1], n_short / n_pairs
