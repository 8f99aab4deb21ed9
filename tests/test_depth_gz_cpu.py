"""The compressed-domain read of this project's own .depth.gz without a GPU: the CPU twin of k_depth_gz.hip (gci_depth_gz_scan / _runs /
_expand in libgci_cpu.so) against zlib on the members CpuEngine.depth_deflate writes and on forged members outside the grammar, its
termination on candidates that are no member starts, the host's chain over the twin with its whole-file fall-backs, and the twin
under AddressSanitizer + UBSan in a stand-alone program."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import depth_gz_cases as cases
from gci_amd import phases, pipeline
from gci_amd.cpu import CpuEngine
from gci_amd.formats import depthfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = CpuEngine()
    yield e
    e.close()


def _raw(data) -> np.ndarray:
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _scan_one(eng, data: bytes):
    return eng.depth_gz_scan(_raw(data), np.zeros(1, dtype=np.uint64))[0]


def _runs_one(eng, data: bytes, info) -> np.ndarray:
    m = np.zeros(1, dtype=depthfile.DGZ_MEMBER_DTYPE)
    m["runs"], m["lines"] = info["runs"], info["lines"]
    return eng.depth_gz_runs(_raw(data), m)[:int(info["runs"])]


def test_twin_agrees_with_zlib_on_every_member_the_writer_makes(eng):
    lengths, track, offsets, data = cases.member_set()
    raw = _raw(data)
    cand = depthfile.member_candidates(data)
    info = eng.depth_gz_scan(raw, cand)
    chain = depthfile.member_chain(data, cand, info)
    assert chain is not None
    names, got_lengths, members = chain
    assert got_lengths == lengths and names == ["ctg%d" % c for c in range(len(lengths))]
    table = depthfile.place_members(members, offsets)
    assert table.shape[0] == sum((L + 64 * 4096 - 1) // (64 * 4096) for L in lengths)
    by_pos = {int(p): k for k, p in enumerate(cand.tolist())}
    runs = eng.depth_gz_runs(raw, table)
    widths = set()
    for m in table:
        pos, i = int(m["pos"]), info[by_pos[int(m["pos"])]]
        text, used = cases.zlib_member(data[pos:])                      # zlib checks CRC-32 and ISIZE itself
        assert (int(i["status"]), int(i["end"]), int(i["lines"])) == (depthfile.DGZ_OK, pos + used, text.count(b"\n"))
        assert i["crc_ok"] == 1 and i["isize_ok"] == 1
        mine = runs[int(m["run0"]):int(m["run0"]) + int(m["runs"])]
        want = track[int(m["elem0"]):int(m["elem0"]) + int(m["lines"])]
        assert np.array_equal(np.repeat(mine["depth"], mine["count"]), want)
        assert np.array_equal(np.array(text.split(b"\n")[:-1], dtype=np.int64), want)
        widths |= {len(b"%d\n" % v) for v in np.unique(want)}
    assert widths >= set(range(2, 12))
    out = np.full(track.shape[0], -1, dtype=np.int32)
    eng.depth_gz_expand(runs, table, out)
    inside = np.zeros(track.shape[0], dtype=bool)
    for o, L in zip(offsets, lengths):
        inside[o:o + L] = True
    assert np.array_equal(out[inside], track[inside]) and (out[~inside] == -1).all()


def test_members_outside_the_grammar_are_refused(eng):
    for name, (data, text) in cases.outside_grammar().items():
        assert cases.zlib_member(data) == (text, len(data)), name       # a legal gzip member, all of it
        i = _scan_one(eng, data)
        assert int(i["status"]) == depthfile.DGZ_FOREIGN, name
        assert (int(i["end"]), int(i["lines"]), int(i["runs"]), int(i["crc_ok"]), int(i["isize_ok"])) == (0, 0, 0, 0, 0), name
    data, text = cases.over_the_line_cap()
    assert cases.zlib_member(data) == (text, len(data)) and int(_scan_one(eng, data)["status"]) == depthfile.DGZ_FOREIGN


def test_forged_members_inside_the_grammar_decode_to_zlibs_text(eng):
    for name, (data, text) in cases.inside_grammar().items():
        assert cases.zlib_member(data) == (text, len(data)), name
        i = _scan_one(eng, data)
        assert (int(i["status"]), int(i["end"]), int(i["lines"])) == (depthfile.DGZ_OK, len(data), text.count(b"\n")), name
        assert i["crc_ok"] == 1 and i["isize_ok"] == 1, name
        assert cases.text_of_runs(_runs_one(eng, data, i)) == text, name


def test_a_wrong_crc_or_isize_is_reported_and_sends_the_file_to_the_text_path(eng):
    for which, (data, text) in cases.off_by_one().items():
        assert cases.zlib_member(data) is None                          # zlib refuses it
        i = _scan_one(eng, data)
        assert int(i["status"]) == depthfile.DGZ_OK and int(i["end"]) == len(data)
        assert (int(i["crc_ok"]), int(i["isize_ok"])) == ((0, 1) if which == "crc" else (1, 0))
        whole = cases.header_member("a") + data
        cand = depthfile.member_candidates(whole)
        assert depthfile.member_chain(whole, cand, eng.depth_gz_scan(_raw(whole), cand)) is None


def test_random_forged_members_are_refused_or_decoded_exactly(eng):
    """No forged legal member is accepted with values other than zlib's."""
    rng = np.random.default_rng(9)
    accepted = refused = 0
    for _ in range(300):
        tokens = []
        for _ in range(int(rng.integers(1, 6))):
            v = int(rng.choice(cases.VALUES + [5, 99, 100]))
            tokens += cases.run_tokens(v, int(rng.integers(1, 400)), rng)
        if rng.random() < 0.6:                                          # one token changed: a distance, a length, a digit
            k = int(rng.integers(0, len(tokens)))
            t = tokens[k]
            if isinstance(t, tuple):
                tokens[k] = (t[0], max(1, t[1] + int(rng.choice([-1, 1])))) if rng.random() < 0.5 else (int(rng.integers(3, 259)), t[1])
            else:
                tokens[k] = int(rng.choice([48, 49, 57, 10]))
        data, text = cases.member([cases.forge.Fixed(tokens)])
        if cases.zlib_member(data) != (text, len(data)):
            continue                                                    # (a distance beyond the start of the text)
        i = _scan_one(eng, data)
        if int(i["status"]) == depthfile.DGZ_OK:
            assert i["crc_ok"] == 1 and i["isize_ok"] == 1 and int(i["end"]) == len(data)
            assert cases.text_of_runs(_runs_one(eng, data, i)) == text
            accepted += 1
        else:
            refused += 1
    assert accepted >= 50 and refused >= 50


def test_every_candidate_returns_and_none_ends_beyond_the_buffer():
    eng = CpuEngine(threads=1)
    data = cases.layout_200()[4]
    data = data[:20_000]
    n = len(data)
    ok = 0
    for o in range(n):                                                  # the header stamped at every byte offset
        i = eng.depth_gz_scan(_raw(cases.stamped(data, [o])), np.array([o], dtype=np.uint64))[0]
        assert int(i["end"]) <= n
        ok += int(i["status"]) == depthfile.DGZ_OK
    assert ok >= 10                                                     # (the true member starts among them)
    cand = depthfile.member_candidates(data)
    info = eng.depth_gz_scan(_raw(data), cand)
    k = int(np.flatnonzero(info["status"] == depthfile.DGZ_OK)[-1])
    whole = data[int(cand[k]):int(info["end"][k])]
    for cut in range(1, 65):                                            # a member truncated at every byte of its last 64
        i = _scan_one(eng, whole[:len(whole) - cut])
        assert int(i["status"]) == depthfile.DGZ_FOREIGN and int(i["end"]) == 0
    eng.close()


def _plan(eng, data, path="f.depth.gz"):
    phases.start()
    try:
        plan = pipeline.depth_members_plan(eng, path, bytearray(data), lambda b: np.frombuffer(b, dtype=np.uint8))
        return plan, phases.report()["notes"]["depth_read:" + path]
    finally:
        phases.stop()


def test_host_chain_over_the_twin_equals_the_text_reader(eng, tmp_path, monkeypatch):
    monkeypatch.delenv("GCI_DEPTH_READ", raising=False)
    names, lengths, track, offsets, data = cases.layout_200()
    path = str(tmp_path / "own.depth.gz")
    with open(path, "wb") as f:
        f.write(data)
    plan, note = _plan(eng, data)
    assert note == "members"
    (got_names, got_lengths, members), raw = plan
    table = depthfile.place_members(members, offsets)
    assert table.shape[0] + len(names) >= 400
    out = np.zeros(track.shape[0], dtype=np.int32)
    eng.depth_gz_track(raw, table, out)
    want = depthfile.read_depth_gz(path)
    assert got_names == list(want) and got_lengths == [len(a) for a in want.values()] == lengths
    for o, (nm, a) in zip(offsets, want.items()):
        assert np.array_equal(out[o:o + len(a)], a), nm
    monkeypatch.setenv("GCI_DEPTH_READ", "text")
    assert _plan(eng, data) == (None, "text")
    monkeypatch.setenv("GCI_DEPTH_READ", "neither")
    with pytest.raises(ValueError):
        _plan(eng, data)


def test_whole_file_fall_backs(eng, monkeypatch):
    monkeypatch.delenv("GCI_DEPTH_READ", raising=False)
    names, lengths, track, offsets, data = cases.layout_200()
    cand = depthfile.member_candidates(data)
    first_data = int(cand[0])
    e = CpuEngine()
    e.set_layout([3])
    one = bytes(e.depth_deflate(np.array([4, 4, 9] + [0] * (e.total - 3), dtype=np.int32))[0])
    e.close()
    text = b"".join(b">%s\n" % nm.encode() + b"".join(b"%d\n" % v for v in track[o:o + L]) for nm, o, L in
                    zip(names[:5], offsets, lengths))
    files = {
        "NUL padding": data + b"\0" * 512,
        "a repeated name": data + cases.header_member(names[3]) + one,
        "a header member holding two lines": data + gzip.compress(b">extra\n5\n"),
        "the reference's gzip": gzip.compress(text),
        "data in front of the first header": data[first_data:],
        "a header without lines at the end": data + cases.header_member("last"),
        "a damaged member": data[:first_data + 40] + bytes([data[first_data + 40] ^ 0x55]) + data[first_data + 41:],
        "an empty file": b"",
    }
    for what, blob in files.items():
        assert _plan(eng, blob) == (None, "text"), what
    assert _plan(eng, data + cases.header_member("one_more") + one)[1] == "members"


def test_twin_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "depth_gz_fuzz")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-o", exe, os.path.join(ROOT, "tests", "depth_gz_fuzz_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    data = cases.layout_200()[4]
    data = data[:20_000]
    cand = depthfile.member_candidates(data)
    e = CpuEngine(threads=1)
    info = e.depth_gz_scan(_raw(data), cand)
    e.close()
    k = int(np.flatnonzero(info["status"] == depthfile.DGZ_OK)[-1])
    src = tmp_path / "members.bin"
    src.write_bytes(data)
    r = subprocess.run([exe, str(src), str(int(cand[k])), str(int(info["end"][k]))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("accepted ") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
