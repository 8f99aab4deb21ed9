"""gci_amd/csrc/gci_deflate_codes.hpp -- the Huffman code set both GPU inflaters (k_inflate.hip, k_inflate_wave.hip) are built on --
held to account without a GPU: the header compiled for the host into deflate_codes_check.cpp, which decodes BGZF members serially
with the header's build_code, build_table and limits search and holds every member against zlib, every table filled entry by entry
against build_table, every long code's entry against the search, and the forged code sets of forge_cases.py against the verdicts
zlib gives (test_deflate_forge_cpu.py proves zlib's side on the same cases).  Once more under AddressSanitizer and UBSan: a
stand-alone host program, nothing loaded into python."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import forge_cases as fc
from deflate_forge import bgzf_member
from gci_amd import synth
from gci_amd.formats import bam as bamfmt
from gci_amd.formats import bgzf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGAL = ("header_extremes", "few_dist_codes", "skewed_lit", "long_used_codes", "lit_tail_overflow")
MALFORMED = ("over_subscribed", "incomplete")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the BAM of the old wave-scheme test with its three odd members behind it; the legal and the malformed forged members"""
    d = tmp_path_factory.mktemp("deflate_codes")
    rs = synth.simulate_reads((("chr19", 400_000),), 40, "hifi", seed=synth.seed_for(2, 0))
    stream, _ = synth.to_bam_stream(rs, seq_qual="random", seed=7)
    p = str(d / "x.bam")
    bamfmt.write_bam_stream(p, stream, level=1, threads=2)
    # members of other kinds behind it: stored blocks (level 0), fixed-code blocks (tiny payloads), an empty member
    with open(p, "ab") as f:
        for payload, level in ((bytes(np.random.default_rng(1).integers(0, 256, 40000, dtype=np.uint8)), 0), (b"ACGT" * 9, 9), (b"", 6)):
            f.write(bgzf._member(payload, level))
    out = {"bam": p}
    legal = [c for name in LEGAL for c in fc.legal_cases(name)]
    bad = [c for name in MALFORMED for c in fc.malformed_cases()[name]]
    assert len(legal) >= 25 and len(bad) >= 10
    for key, cases in (("legal", legal), ("malformed", bad)):
        out[key] = str(d / (key + ".bgzf"))
        with open(out[key], "wb") as f:
            for c in cases:
                f.write(bgzf_member(c.data, c.payload, isize=c.isize))
        out["n_" + key] = len(cases)
    return out


BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """the check program in both builds; every test below runs both and asserts the same of each"""
    d = tmp_path_factory.mktemp("build")
    out = []
    for name, flags in BUILDS.items():
        out.append(str(d / ("check_" + name)))
        subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", out[-1], os.path.join(ROOT, "tests", "deflate_codes_check.cpp"), "-lz"])
    return out


def run(exes, path, mode):
    """what the program reports of `path`, the same from the plain and from the sanitized build"""
    seen = []
    for exe in exes:
        r = subprocess.run([exe, path, mode], capture_output=True, text=True)
        assert r.returncode == 0, exe + ": " + r.stderr[-2000:]
        m = re.match(r"(\d+) members (.*), (\d+) blocks with their tables, (\d+) code values", r.stdout)
        assert m, r.stdout
        seen.append((int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))))
    assert len(seen) == len(BUILDS) and all(s == seen[0] for s in seen), seen
    return seen[0]


def test_every_member_of_a_bam_equals_zlib(exes, files):
    members, what, blocks, values = run(exes, files["bam"], "accept")
    assert what == "equal to zlib byte for byte"
    assert members > 300 and blocks >= members - 2 and values > 0          # (all but the stored and the empty member have a coded block)


def test_legal_forged_code_sets_decode_to_their_payload(exes, files):
    members, what, blocks, values = run(exes, files["legal"], "accept")
    assert what == "equal to zlib byte for byte" and members == files["n_legal"] and blocks >= members and values > 0


def test_malformed_code_sets_are_refused_by_build_code(exes, files):
    members, what, _, _ = run(exes, files["malformed"], "refuse")
    assert what == "refused by build_code and by zlib" and members == files["n_malformed"]
