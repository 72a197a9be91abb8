"""csrc/wr_lin_host.cpp with csrc/wr_host.cpp and csrc/graph_host.cpp:
tests/wr_lin_main.cpp built with g++ and the address and undefined-behaviour
sanitizers, run as a child process (as tests/test_wr_host_sanitize.py runs
its program).  The program checks the hand-derived histories' arrays under all
four flag combinations, and histories it generates of up to 1,500 txns, every
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
KATS = json.load(open(os.path.join(HERE, "golden", "wr_lin_kat.json")))["cases"]
FIELDS = (("valid", "valid"), ("cyclic", "n_cyclic_keys"), ("phantom", "n_phantom"), ("keys", "n_keys"),
          ("edges", "n_edges"), ("raw", "n_edges_raw"), ("scc", "n_scc"))
LIN_FIELDS = (("touches", "n_touches"), ("pairs", "n_pairs"), ("vedges", "n_vedges"), ("maxv", "max_key_versions"))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    tmp = tmp_path_factory.mktemp("wr_lin")
    exe, cases = str(tmp / "wr_lin_main"), str(tmp / "cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<q", 4 * len(KATS)))
        for kat in KATS:
            enc = WR.encode(kat["history"])
            for flags in range(4):
                f.write(struct.pack("<qqq", len(enc.txns), len(enc.mops), flags))
                f.write(enc.txns.tobytes())
                f.write(enc.mops.tobytes())
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(HERE, "wr_lin_main.cpp"), os.path.join(CSRC, "wr_lin_host.cpp"),
                           os.path.join(CSRC, "wr_host.cpp"), os.path.join(CSRC, "graph_host.cpp"), "-o", exe])
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        out.append((f[0], int(f[1]), dict(zip(f[2::2], f[3::2]))))
    return out


def test_kats_under_the_sanitizers_give_the_library_s_counts(lines):
    cases = [rec for name, _, rec in lines if name == "case"]
    assert len(cases) == 4 * len(KATS)
    for i, kat in enumerate(KATS):
        enc = WR.encode(kat["history"])
        for flags in range(4):
            _, s, ls = abi.wr_check_lin_host(enc.txns, enc.mops, bool(flags & 1), bool(flags & 2))
            rec = cases[4 * i + flags]
            assert int(rec["rc"]) == 0, (kat["name"], flags)
            assert [int(rec[a]) for a, _ in FIELDS] == [s[b] for _, b in FIELDS], (kat["name"], flags, rec, s)
            assert [int(rec[a]) for a, _ in LIN_FIELDS] == [ls[b] for _, b in LIN_FIELDS], (kat["name"], flags, rec, ls)


def test_generated_histories_ran_and_met_the_shapes(lines):
    gen = [rec for name, _, rec in lines if name == "gen"]
    assert len(gen) == 32 and all(int(rec["rc"]) == 0 for rec in gen)
    with_lin = [rec for i, rec in enumerate(gen) if i % 4 >= 2]
    for field in ("cyclic", "phantom", "scc", "pairs"):
        assert any(int(rec[field]) > 0 for rec in with_lin), field
    assert all(int(rec["pairs"]) == 0 and int(rec["touches"]) == 0 for i, rec in enumerate(gen) if i % 4 < 2)
    assert any(int(rec["pairs"]) > 4 * int(rec["touches"]) > 0 for rec in with_lin)   # long successor runs
    assert any(int(rec["maxv"]) > 64 for rec in with_lin)
    # (most generated keys are cyclic under the inference and keep their wr edges alone)
    assert all(int(rec["raw"]) >= int(rec["edges"]) for rec in gen) and any(int(rec["edges"]) > 100 for rec in with_lin)
    assert int(gen[0]["valid"]) == -1  # no txns


def test_refusals(lines):
    refused = {name: int(rec["rc"]) for name, _, rec in lines if name in ("twice", "tiling", "flags")}
    assert refused == {"twice": -22, "tiling": -22, "flags": -22}
