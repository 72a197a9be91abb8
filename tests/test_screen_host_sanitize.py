"""csrc/screen_host.cpp: tests/screen_main.cpp built with g++ and the address
and undefined-behaviour sanitizers, run as a child process (as
tests/test_wr_host_sanitize.py runs its program).  The program checks the
KATs' arrays and graphs it generates, of up to 1,500 txns, every output array
sized exactly; its lines carry each call's counts, which must be those the
library gives through the binding."""
import json
import os
import shutil
import struct
import subprocess

import pytest

from jepsen.etcd_amd import abi
from test_screen import KATS, arrays

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "jepsen", "etcd_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    tmp = tmp_path_factory.mktemp("screen")
    exe, cases = str(tmp / "screen_main"), str(tmp / "cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<q", len(KATS)))
        for kat in KATS:
            txns, edges = arrays(kat["txns"], kat["edges"])
            f.write(struct.pack("<qq", len(txns), len(edges)))
            f.write(txns.tobytes())
            f.write(edges.tobytes())
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(HERE, "screen_main.cpp"), os.path.join(CSRC, "screen_host.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "LC_SCREEN_MAX_ROUNDS"}
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        out.append((f[0], int(f[1]), dict(zip(f[2::2], (int(x) for x in f[3::2])))))
    return out


def test_kats_under_the_sanitizers_give_the_library_s_counts(lines):
    cases = [rec for name, _, rec in lines if name == "case"]
    assert len(cases) == len(KATS)
    for kat, rec in zip(KATS, cases):
        out, s = abi.cycle_screen_host(*arrays(kat["txns"], kat["edges"]))
        assert rec["rc"] == 0, kat["name"]
        assert [rec[k] for k in ("clean", "rt", "trim", "label_rounds", "trim_rounds", "max_rounds")] == \
            [s[k] for k in ("clean", "n_rt_members", "n_trim_survivors", "label_rounds", "trim_rounds",
                            "max_rounds")], (kat["name"], rec, s)
        assert rec["clean"] == kat["clean"]
        assert (rec["lo"], rec["hi"], rec["marks"]) == (int((out["reach_lo"].astype(int) % 1000).sum()),
                                                        int(out["reach_hi"].sum()), int(out["mark"].sum()))


def test_generated_graphs_ran_and_met_every_kind(lines):
    gen = [rec for name, _, rec in lines if name == "gen"]
    assert len(gen) == 12 and all(rec["rc"] == 0 for rec in gen)
    assert gen[0]["clean"] == 1 and gen[0]["label_rounds"] == 0      # no txns
    assert any(rec["clean"] == 1 and rec["label_rounds"] >= 1 for rec in gen)
    assert any(rec["clean"] == 0 and rec["rt"] > 0 for rec in gen)
    assert any(rec["trim"] > 0 for rec in gen)
    assert any(rec["clean"] == -1 for rec in gen)                    # one that gave up
    assert any(rec["label_rounds"] > 2 for rec in gen) and any(rec["trim_rounds"] > 2 for rec in gen)


def test_refusals(lines):
    refused = {name: rec["rc"] for name, _, rec in lines if name in ("unsorted-txns", "unsorted-edges",
                                                                      "edge-out-of-range")}
    assert refused == {"unsorted-txns": -22, "unsorted-edges": -22, "edge-out-of-range": -22}
