"""What the cross-file join does with every record, and why -- the statement of include/gci_hip.h (gci_name_join_fate,
gci_fate_refine) as per-name Python over arrays of REC_DTYPE records and their names.  A file here is (records, names): names[i] the
bytes of the query name of the record at position i.

For a read name q (the device tells names apart by their hash, their length and their bytes, so the key here is (hash, bytes)):
present[f] = q has a PASS record in file f; the file's winner is the PASS record last in (contig index, position); hq = any PASS
record of q anywhere carries HQ; comm = present in every file.  One file: every name is `joined`.  Several: have = present[0] and
(hq or comm), why = unpaired; files 1 .. n - 1 in order, where q is present: with have -- another contig: have = false, why =
contig; else ovlp / qlen < ovlp_percent (qlen: this file's winner's): have = false, why = overlap; else intersect -- and without
have, with hq: have = true with this winner's interval.  A zero qlen where the quotient is asked for reports ZERO_DIV with the
winner's rec_idx, ends the name's fold and leaves it `overlap`.  A PASS record that is not its file's winner is `shadowed`, a
winner carries its name's verdict, any other record 0."""
import numpy as np

from gci_amd.cpu import REC_DTYPE

PASS, HQ = 1, 2
KEPT = 6
SHADOWED, UNPAIRED, CONTIG, OVERLAP, JOINED = 8, 9, 10, 11, 12
NAMES = ("shadowed", "unpaired", "contig", "overlap", "joined")
ROW = 16                                               # GCI_JOIN_FATE_CLASSES
NO_STATUS = 2 ** 64 - 1
E_INVALID, E_ZERO_DIV = -1, -4


def word(rec, code):
    return (int(rec) << 8) | (-code & 0xFF)


def key_of(recs, names, i):
    return (int(recs["name_hash"][i]), bytes(names[i]))


def winners(recs, names):
    """-> {key: position of the file's winner}, hq keys: the PASS record last in (contig as the device orders it, position)."""
    win, hq = {}, set()
    for i in range(recs.shape[0]):
        if not int(recs["flags"][i]) & PASS:
            continue
        k = key_of(recs, names, i)
        order = (int(recs["contig"][i]) & 0xFFFFFFFF, i)
        if k not in win or order > win[k][0]:
            win[k] = (order, i)
        if int(recs["flags"][i]) & HQ:
            hq.add(k)
    return {k: v[1] for k, v in win.items()}, hq


def statement(files, ovlp_percent):
    """-> (bytes per file [uint8 arrays], counts uint64 [n_files, ROW], status word, {key: (contig, start, end)} of the joined names)."""
    n = len(files)
    win, hq = [], set()
    for recs, names in files:
        w, h = winners(recs, names)
        win.append(w)
        hq |= h
    status = NO_STATUS
    verdict, kept = {}, {}
    for k in set().union(*[set(w) for w in win]):
        seg = lambda f: tuple(int(files[f][0][fld][win[f][k]]) for fld in ("contig", "start", "end", "qlen", "rec_idx"))   # noqa: E731
        if n == 1:
            verdict[k], kept[k] = JOINED, seg(0)[:3]
            continue
        comm = all(k in w for w in win)
        have = k in win[0] and (k in hq or comm)
        why = UNPAIRED
        cur = seg(0)[:3] if have else None
        for f in range(1, n):
            if k not in win[f]:
                continue
            c, s, e, qlen, rec_idx = seg(f)
            if have:
                if c != cur[0]:
                    have, why = False, CONTIG
                    continue
                ms, me = max(s, cur[1]), min(e, cur[2])
                if qlen == 0:
                    status = min(status, word(rec_idx, E_ZERO_DIV))
                    have, why = False, OVERLAP
                    break
                if (me - ms) / qlen < ovlp_percent:
                    have, why = False, OVERLAP
                else:
                    cur = (c, ms, me)
            elif k in hq:
                have, cur = True, (c, s, e)
        verdict[k] = JOINED if have else why
        if have:
            kept[k] = cur
    out, counts = [], np.zeros((n, ROW), dtype=np.uint64)
    for f, (recs, names) in enumerate(files):
        b = np.zeros(recs.shape[0], dtype=np.uint8)
        for i in range(recs.shape[0]):
            if int(recs["flags"][i]) & PASS:
                k = key_of(recs, names, i)
                b[i] = verdict[k] if win[f][k] == i else SHADOWED
        out.append(b)
        counts[f] = np.bincount(b, minlength=ROW)
    return out, counts, status, kept


def refine(classes, join_fate):
    """gci_fate_refine -> (the classes after it, status word)."""
    out, status = np.array(classes, dtype=np.uint8), NO_STATUS
    for i, (c, j) in enumerate(zip(out.tolist(), np.asarray(join_fate).tolist())):
        if c == KEPT and SHADOWED <= j <= JOINED:
            out[i] = j
        elif c == KEPT or j != 0:
            status = min(status, word(i, E_INVALID))
    return out, status


def as_input(recs, names):
    """A file as the join's input: (records, names blob, offsets by position, name_delta)."""
    lens = np.array([len(x) for x in names], dtype=np.uint64)
    off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return np.ascontiguousarray(recs, dtype=REC_DTYPE), np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8), off[:-1].copy(), 0
