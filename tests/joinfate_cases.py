"""The cases of the join's record verdicts (tests/joinfate_ref.py holds the statement): hand cases of a few records each, the sizes
at which the table and the grids change, and randomised sets.  A case is dict(files=[(records, names)], ops=[ovlp_percent, ...]);
want(name, op) is the statement's answer, computed once."""
import numpy as np

import joinfate_ref as J
from gci_amd.cpu import REC_DTYPE
from gci_amd.device import name_hash_np

P, H = J.PASS, J.PASS | J.HQ
MAX_FILES = 16


def mk(*rows):
    """rows of (name, contig, start, end, qlen, flags[, forged hash[, rec_idx]]) -> (records, names); rec_idx = position unless given."""
    names = [r[0] for r in rows]
    recs = np.zeros(len(rows), dtype=REC_DTYPE)
    if rows:
        recs["name_hash"] = name_hash_np(names)
    for i, r in enumerate(rows):
        recs["contig"][i], recs["start"][i], recs["end"][i], recs["qlen"][i], recs["flags"][i] = r[1:6]
        recs["name_len"][i] = len(r[0])
        recs["rec_idx"][i] = r[7] if len(r) > 7 else i
        recs["mapq"][i] = 60 if r[5] & J.HQ else 20
        if len(r) > 6 and r[6] is not None:
            recs["name_hash"][i] = r[6]
    return recs, names


def _hand():
    up, down = float(np.nextafter(0.9, 1.0)), float(np.nextafter(0.9, 0.0))
    c = {}
    # the quotient on, just below and just above -op: ovlp 9, 8 and 10 over qlen 10; and -op one ulp beside 0.9
    c["quotient"] = dict(ops=[0.9, up, down], files=[
        mk((b"on", 0, 0, 100, 50, H), (b"below", 0, 1000, 1100, 50, H), (b"above", 0, 2000, 2100, 50, H)),
        mk((b"on", 0, 91, 200, 10, P), (b"below", 0, 1092, 1200, 10, P), (b"above", 0, 2090, 2200, 10, P))])
    c["disjoint"] = dict(ops=[0.9, 0.0, -1.0], files=[mk((b"q", 0, 0, 100, 100, H)), mk((b"q", 0, 150, 250, 100, H))])
    c["other_contig"] = dict(ops=[0.9], files=[mk((b"q", 0, 0, 100, 100, H), (b"r", 1, 0, 100, 100, P)),
                                               mk((b"q", 1, 0, 100, 100, H), (b"r", 1, 0, 100, 100, P))])
    # hq only on a record its file's dict overwrites: the name still counts as high quality
    c["hq_shadowed"] = dict(ops=[0.9], files=[mk((b"q", 0, 0, 100, 100, H), (b"q", 0, 500, 600, 100, P), (b"r", 0, 0, 100, 100, P),
                                                 (b"r", 0, 500, 600, 100, P)),
                                              mk((b"other", 0, 0, 100, 100, P))])
    c["hq_absent_from_file0"] = dict(ops=[0.9], files=[mk((b"x", 0, 0, 10, 10, P)), mk((b"q", 1, 7, 70, 63, H), (b"low", 1, 7, 70, 63, P))])
    three = [mk((b"q", 0, 100, 200, 100, P), (b"n", 0, 100, 200, 100, P)), mk((b"q", 1, 100, 200, 100, P), (b"n", 1, 100, 200, 100, P)),
             mk((b"q", 2, 300, 400, 100, H), (b"n", 2, 300, 400, 100, P))]
    c["delete_resurrect"] = dict(ops=[0.9], files=three)
    c["delete_resurrect_delete"] = dict(ops=[0.9, 0.1], files=three + [mk((b"q", 2, 380, 480, 100, P), (b"n", 2, 380, 480, 100, P))])
    # the winner is by contig first: the record on the higher contig index comes EARLIER in the file and still wins
    c["winner_by_contig"] = dict(ops=[0.9], files=[mk((b"q", 1, 50, 150, 100, H), (b"q", 0, 50, 150, 100, H)),
                                                   mk((b"q", 1, 50, 150, 100, P))])
    c["forged_hash_same_length"] = dict(ops=[0.9], files=[mk((b"aaaa", 0, 0, 100, 100, H, 0x1234), (b"bbbb", 0, 0, 100, 100, P, 0x1234),
                                                            (b"bbbb", 0, 5, 100, 100, P, 0x1234)),
                                                         mk((b"bbbb", 1, 0, 100, 100, P, 0x1234), (b"aaaa", 0, 0, 100, 100, P, 0x1234))])
    c["forged_hash_other_length"] = dict(ops=[0.9], files=[mk((b"aaaa", 0, 0, 100, 100, H, 0x77), (b"aaaaa", 0, 0, 100, 100, P, 0x77)),
                                                          mk((b"aaaaa", 0, 300, 400, 100, P, 0x77), (b"aaaa", 0, 0, 100, 100, P, 0x77))])
    c["not_pass_interleaved"] = dict(ops=[0.9], files=[
        mk((b"q", 0, 0, 100, 100, 0), (b"q", 0, 10, 100, 100, P), (b"q", 0, 20, 100, 100, J.HQ), (b"r", 0, 0, 9, 9, 0), (b"s", 0, 0, 50, 50, P),
           (b"q", 1, 0, 100, 100, 0)),
        mk((b"s", 0, 0, 50, 50, 0), (b"q", 0, 10, 100, 100, P), (b"r", 0, 0, 9, 9, P))])
    # a zero qlen the quotient meets (two of them: the smaller word is reported), and where it does not: in file 0, behind another
    # contig, on a name that is not held
    c["zero_qlen_reached"] = dict(ops=[0.9], files=[mk((b"a", 0, 0, 100, 0, H), (b"b", 0, 0, 100, 100, H), (b"c", 0, 0, 100, 100, H)),
                                                   mk((b"a", 0, 0, 100, 100, P, None, 40), (b"b", 0, 0, 100, 0, P, None, 41),
                                                      (b"c", 0, 0, 100, 0, P, None, 7))])
    c["zero_qlen_not_reached"] = dict(ops=[0.9], files=[mk((b"a", 0, 0, 100, 0, H), (b"b", 0, 0, 100, 100, H)),
                                                       mk((b"a", 0, 0, 100, 100, P), (b"b", 1, 0, 100, 0, P), (b"low", 0, 0, 100, 0, P))])
    c["one_file"] = dict(ops=[0.9], files=[mk((b"q", 0, 0, 100, 100, P), (b"r", 0, 0, 100, 0, 0), (b"q", 0, 5, 100, 100, P), (b"t", 1, 0, 100, 100, H))])
    c["empty_file_of_three"] = dict(ops=[0.9], files=[mk((b"q", 0, 0, 100, 100, H), (b"n", 0, 0, 100, 100, P)), mk(),
                                                     mk((b"q", 0, 0, 100, 100, P), (b"n", 0, 0, 100, 100, P))])
    c["max_files"] = dict(ops=[0.9], files=[mk((b"q", 0, f, 200 - f, 100, P), (b"h", f % 2, 0, 100, 100, H if f == 3 else P),
                                               *([(b"gap", 0, 0, 100, 100, P)] if f != 9 else [])) for f in range(MAX_FILES)])
    c["three_records"] = dict(ops=[0.9], files=[mk((b"q", 0, 0, 100, 100, P)), mk((b"q", 0, 0, 100, 100, P), (b"z", 0, 0, 1, 1, H))])
    return c


def _sized():
    """513 passing records in file 0: the table leaves its 1024 slots, the per-slot kernels take more than one workgroup."""
    names = [b"read%04d" % i for i in range(513)]
    f0 = mk(*[(n, i % 3, 10 * i, 10 * i + 500, 500, H if i % 5 == 0 else P) for i, n in enumerate(names)])
    f1 = mk(*[(n, (i + (i % 11 == 0)) % 3, 10 * i + (i % 7) * 20, 10 * i + 500, 500, P) for i, n in enumerate(names) if i % 4 != 1])
    return {"slots_2048": dict(ops=[0.9], files=[f0, f1])}


def _random(seed, n_files, n_recs=5000, pool=600):
    """About n_recs records over n_files files from a pool of names; a tenth of the pool shares forged hashes in threes, another tenth
    the low bits of its hash (one probe chain)."""
    rng = np.random.default_rng(seed)
    names = [b"m%03d/%d/ccs" % (i, 17 * i) for i in range(pool)]
    hashes = name_hash_np(names)
    hashes[:pool // 10] = 0xC0FFEE00 + np.arange(pool // 10, dtype=np.uint64) // 3
    hashes[pool // 10:pool // 5] = (hashes[pool // 10:pool // 5] & ~np.uint64(0xFFFF)) | np.uint64(0x1F3)
    home_c, home_s = rng.integers(0, 3, pool), rng.integers(0, 90_000, pool)
    length = rng.integers(200, 3000, pool)
    files = []
    for f in range(n_files):
        per = n_recs // n_files
        pick = rng.integers(0, pool, per)
        u = rng.random(per)
        contig = np.where(u < 0.05, (home_c[pick] + 1) % 3, home_c[pick])
        start = home_s[pick] + np.where(u < 0.25, rng.integers(-400, 400, per), 0)
        flags = np.where(rng.random(per) < 0.08, 0, np.where(rng.random(per) < 0.45, H, P))
        rows = [(names[p], int(contig[k]), int(start[k]), int(start[k] + length[p]), int(length[p] + rng.integers(-20, 200)), int(flags[k]),
                 int(hashes[p])) for k, p in enumerate(pick.tolist())]
        files.append(mk(*rows))
    return dict(ops=[0.9], files=files)


CASES = {}
CASES.update(_hand())
CASES.update(_sized())
for _n in range(1, 6):
    CASES["random_%d_files" % _n] = _random(40 + _n, _n)
NAMES = list(CASES)
_WANT = {}


def case(name):
    return CASES[name]


def pairs():
    return [(name, op) for name in NAMES for op in CASES[name]["ops"]]


def want(name, op):
    if (name, op) not in _WANT:
        _WANT[(name, op)] = J.statement(CASES[name]["files"], op)
    return _WANT[(name, op)]


def inputs(name):
    return [J.as_input(r, n) for r, n in CASES[name]["files"]]
