"""csrc/wr_host.cpp and the graph code it shares with list-append
(csrc/graph_host.cpp): tests/wr_main.cpp built with g++ and the address and
undefined-behaviour sanitizers, run as a child process (as
tests/test_plan_host.py runs its program).  The program checks the KATs'
arrays, with the wfr inference on and off, and histories it generates, every
output array sized exactly; its lines carry each call's counts, which must be
those the library gives through the binding."""
import json
import os
import shutil
import struct
import subprocess

import pytest

from jepsen.etcd_amd import abi, wr as WR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "jepsen", "etcd_amd", "csrc")
KATS = json.load(open(os.path.join(HERE, "golden", "wr_kat.json")))["cases"]
FIELDS = (("valid", "valid"), ("internal", "n_internal"), ("phantom", "n_phantom"), ("g1a", "n_g1a"),
          ("g1b", "n_g1b"), ("cyclic", "n_cyclic_keys"), ("lost", "n_lost_update"), ("keys", "n_keys"),
          ("versions", "n_versions"), ("ok", "n_ok"), ("nodes", "n_nodes"), ("edges", "n_edges"),
          ("raw", "n_edges_raw"), ("scc", "n_scc"))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    tmp = tmp_path_factory.mktemp("wr")
    exe, cases = str(tmp / "wr_main"), str(tmp / "cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<q", 2 * len(KATS)))
        for kat in KATS:
            enc = WR.encode(kat["history"])
            for flags in (abi.LC_WR_WFR_KEYS, 0):
                f.write(struct.pack("<qqq", len(enc.txns), len(enc.mops), flags))
                f.write(enc.txns.tobytes())
                f.write(enc.mops.tobytes())
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(HERE, "wr_main.cpp"), os.path.join(CSRC, "wr_host.cpp"),
                           os.path.join(CSRC, "graph_host.cpp"), "-o", exe])
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        out.append((f[0], int(f[1]), dict(zip(f[2::2], f[3::2]))))
    return out


def test_kats_under_the_sanitizers_give_the_library_s_counts(lines):
    cases = [rec for name, _, rec in lines if name == "case"]
    assert len(cases) == 2 * len(KATS)
    for i, kat in enumerate(KATS):
        enc = WR.encode(kat["history"])
        for j, wfr in enumerate((True, False)):
            _, s = abi.wr_check_host(enc.txns, enc.mops, wfr)
            rec = cases[2 * i + j]
            assert int(rec["rc"]) == 0, (kat["name"], wfr)
            assert [int(rec[a]) for a, _ in FIELDS] == [s[b] for _, b in FIELDS], (kat["name"], wfr, rec, s)
            assert rec["classes"] == "".join(str(min(n, 9)) for n in s["n_class"]), (kat["name"], wfr)


def test_generated_histories_ran_and_met_the_anomalies(lines):
    gen = [rec for name, _, rec in lines if name == "gen"]
    assert len(gen) == 14 and all(int(rec["rc"]) == 0 for rec in gen)
    for field in ("internal", "phantom", "g1a", "g1b", "cyclic", "lost", "scc"):
        assert any(int(rec[field]) > 0 for rec in gen), field
    assert any(int(rec["raw"]) > int(rec["edges"]) > 10000 for rec in gen)  # the edge buffers grew, unique cut
    assert int(gen[0]["valid"]) == -1  # no txns


def test_refusals(lines):
    refused = {name: int(rec["rc"]) for name, _, rec in lines if name in ("twice", "tiling", "flags")}
    assert refused == {"twice": -22, "tiling": -22, "flags": -22}
