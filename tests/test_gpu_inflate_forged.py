"""Both GPU inflaters (k_inflate_wave.hip with its hand-back, k_inflate.hip alone) on DEFLATE streams zlib's encoder never writes:
the forged classes of forge_cases.py, each stream proven against zlib by test_deflate_forge_cpu.py.  The reference is zlib: a
member is accepted iff zlib inflates its stream without error to the end and to ISIZE bytes, and then the bytes are zlib's.

Every legal class is one file -- its members between ordinary zlib members -- through the default path with and without the CRC
check, and through the lane decoder alone (GCI_INFLATE=lane, read once per process: a child).  Every malformed stream is one bad
member among good ones and one call with the CRC check off: GCI_E_MALFORMED naming that member, from both decoders.
Who decoded what is printed (-s), not asserted: a legal stream the wave decoder hands back is no bug, one the lane decoder refuses is.
"""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import forge_cases as fc
from deflate_forge import bgzf_member
from gci_amd import hostio
from gci_amd._lib import GciError, GCI_E_MALFORMED

pytestmark = pytest.mark.gpu


def table(f):
    buf = np.frombuffer(f.raw, dtype=np.uint8)
    pos, isz = hostio.bgzf_blocks(buf)
    assert [int(x) for x in isz] == [f.forged[m].isize if m in f.forged else len(p) for m, p in enumerate(f.payloads)]
    return buf, pos, isz


def check_file(engine, f, what):
    buf, pos, isz = table(f)
    off = np.concatenate([[0], np.cumsum(isz)]).astype(np.int64)
    want = b"".join(f.payloads)
    for check_crc in (True, False):
        got = engine.bgzf_inflate(buf, pos, isz, check_crc=check_crc).cpu().numpy().tobytes()
        if got != want:
            bad = [m for m in range(len(isz)) if got[off[m]:off[m + 1]] != want[off[m]:off[m + 1]]]
            names = [f.forged[m].name if m in f.forged else "zlib member" for m in bad[:5]]
            pytest.fail("%s, check_crc=%s: %d members differ, first %s: %s" % (what, check_crc, len(bad), bad[:5], names))
        st = engine.inflate_stats()
        assert st["not tried"] == 0 and sum(st.values()) == len(isz), st
    return st


@pytest.mark.parametrize("name", sorted(fc.LEGAL))
def test_legal_streams_inflate_to_zlibs_bytes(engine, name):
    cases = fc.legal_cases(name)
    check_file(engine, fc.build_file(cases), name)
    st = check_file(engine, fc.build_file(cases, neighbours=False), name + " (forged members only)")
    print("\n%s: %d forged members (and the empty last one): %s" % (name, len(cases), st))


def test_zlib_members_with_flushes_and_a_full_member(engine):
    """what zlib CAN write and the suite never asked for: sync, full and partial flushes in mid-payload (empty stored / fixed blocks
    between the others), and ISIZE 65 536"""
    rng = np.random.default_rng(12)
    members, want = [], []
    for n in (0, 1, 700, 30000, 65535, 65536):
        pay = fc.text(rng, n)
        for flush in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, getattr(zlib, "Z_PARTIAL_FLUSH", 1)):
            for level in (1, 6, 9):
                c = zlib.compressobj(level, zlib.DEFLATED, -15)
                cuts = sorted(int(x) for x in rng.integers(0, n + 1, 4))
                body = b"".join(c.compress(pay[a:b]) + c.flush(flush) for a, b in zip([0] + cuts, cuts + [n])) + c.flush()
                if len(body) <= fc.MAX_DEFLATE:
                    members.append(bgzf_member(body, pay)); want.append(pay)
    assert len(members) > 45 and max(len(p) for p in want) == 65536
    st = check_file(engine, fc.File(b"".join(members) + fc.BGZF_EOF, want + [b""], {}), "zlib members with flushes")
    print("\nzlib members with flushes:", st)


@pytest.fixture(scope="module")
def lane_child(tmp_path_factory):
    """every legal file and every malformed one through a process with GCI_INFLATE=lane: the lane decoder sees every stream, not
    only the hand-backs.  The legal files first; a malformed file is run once.  -> what the child printed, per file"""
    d = tmp_path_factory.mktemp("forged")
    jobs = []

    def put(tag, f, bad):
        k = len(jobs)
        np.save(str(d / ("raw%d.npy" % k)), np.frombuffer(f.raw, dtype=np.uint8))
        np.save(str(d / ("want%d.npy" % k)), np.frombuffer(b"".join(f.payloads), dtype=np.uint8))
        jobs.append(dict(tag=tag, k=k, bad=bad))

    for name in sorted(fc.LEGAL):
        put("legal " + name, fc.build_file(fc.legal_cases(name)), None)
    for name, cases in fc.malformed_cases().items():
        for c in cases:
            f = fc.build_file([c])
            put("malformed %s: %s" % (name, c.name), f, next(iter(f.forged)))
    (d / "jobs.json").write_text(json.dumps(jobs))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = d / "run.py"
    script.write_text(
        "import json, sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from gci_amd import hostio\n"
        "from gci_amd._lib import GciError, GCI_E_MALFORMED\n"
        "from gci_amd.device import Engine\n"
        "d = %r\n"
        "e = Engine(0)\n"
        "for j in json.load(open(d + '/jobs.json')):\n"
        "    raw, want = np.load(d + '/raw%%d.npy' %% j['k']), np.load(d + '/want%%d.npy' %% j['k'])\n"
        "    pos, isz = hostio.bgzf_blocks(raw)\n"
        "    for check_crc in ((True, False) if j['bad'] is None else (False,)):\n"
        "        try:\n"
        "            got = e.bgzf_inflate(raw, pos, isz, check_crc=check_crc).cpu().numpy()\n"
        "            res = 'equal' if np.array_equal(got, want) else 'differs'\n"
        "        except GciError as x:\n"
        "            res = 'refused status %%d member %%d' %% (x.status, x.rec)\n"
        "        print(json.dumps(dict(tag=j['tag'], check_crc=check_crc, res=res)), flush=True)\n" % (root, str(d)))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, GCI_INFLATE="lane"), capture_output=True, text=True, timeout=900)
    if r.returncode < 0:                                       # (killed by a signal: nothing more on this GPU in this session)
        pytest.exit("the GCI_INFLATE=lane child died with signal %d: %s" % (-r.returncode, r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            j = json.loads(line)
            out.setdefault(j["tag"], []).append(j["res"])
    return jobs, out


@pytest.mark.parametrize("name", sorted(fc.LEGAL))
def test_the_lane_decoder_alone_inflates_the_legal_streams(lane_child, name):
    jobs, out = lane_child
    assert out["legal " + name] == ["equal", "equal"], out["legal " + name]


def malformed_ids():
    return sorted(fc.MALFORMED_CLASSES)


@pytest.mark.parametrize("name", malformed_ids())
def test_malformed_streams_are_refused(engine, name):
    """one bad member among good ones, the CRC check off, the trailer that of the payload a careless decoder would produce"""
    wrong = []
    for c in fc.malformed_cases()[name]:
        f = fc.build_file([c])
        buf, pos, isz = table(f)
        idx = next(iter(f.forged))
        try:
            engine.bgzf_inflate(buf, pos, isz, check_crc=False)
            wrong.append("%s: accepted" % c.name)
        except GciError as e:
            if e.status != GCI_E_MALFORMED or e.rec != idx:
                wrong.append("%s: status %d, member %d for member %d" % (c.name, e.status, e.rec, idx))
    assert not wrong, "%s (zlib refuses them all): %s" % (name, wrong)


@pytest.mark.parametrize("name", malformed_ids())
def test_the_lane_decoder_alone_refuses_the_malformed_streams(lane_child, name):
    jobs, out = lane_child
    mine = [j for j in jobs if j["tag"].startswith("malformed %s: " % name)]
    assert len(mine) == len(fc.malformed_cases()[name])
    wrong = [(j["tag"], out[j["tag"]]) for j in mine if out[j["tag"]] != ["refused status %d member %d" % (GCI_E_MALFORMED, j["bad"])]]
    assert not wrong, wrong
