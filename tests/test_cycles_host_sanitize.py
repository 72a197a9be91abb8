"""csrc/cycles_host.cpp and csrc/graph_host.cpp: tests/cycles_main.cpp built
with g++ and the address and undefined-behaviour sanitizers, run as a child
process (as tests/test_screen_host_sanitize.py runs its program).  The program
runs lc_cycle_reach_host on the KATs and lc_cycles_host (the whole graph, the
marked pass with the host loop, the marked pass with a hook) on the edges of
the Elle checkers' KATs and on graphs it generates, every output array sized
exactly; its lines carry each call's counts, which must be those the library
gives through the binding.  Nothing is preloaded and nothing runs on a GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from jepsen.etcd_amd import abi, append as AP, wr as WR
from test_append import KATS as AP_KATS
from test_cycles import KATS, kat_arrays
from test_wr import KATS as WR_KATS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "jepsen", "etcd_amd", "csrc")


def graphs():
    """(name, txns, edges) of every Elle KAT: the edges the host checkers build."""
    out = []
    for kat in AP_KATS:
        enc = AP.encode(kat["history"])
        out.append((kat["name"], enc.txns, abi.append_check_host(enc.txns, enc.mops, enc.values)[0]["edges"]))
    for kat in WR_KATS:
        enc = WR.encode(kat["history"])
        out.append((kat["name"], enc.txns, abi.wr_check_host(enc.txns, enc.mops, True)[0]["edges"]))
    return out


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    tmp = tmp_path_factory.mktemp("cycles")
    exe, cases = str(tmp / "cycles_main"), str(tmp / "cases.bin")
    with open(cases, "wb") as f:
        f.write(struct.pack("<q", len(KATS)))
        for kat in KATS:
            n, po, pr, qn, qo, qh = kat_arrays(kat)
            f.write(struct.pack("<qqqq", n, len(pr), len(qn), len(qh)))
            for a, t in ((po, np.int64), (pr, np.int32), (qn, np.int32), (qo, np.int64), (qh, np.int32)):
                f.write(np.asarray(a, dtype=t).tobytes())
        gs = graphs()
        f.write(struct.pack("<q", len(gs)))
        for _, txns, edges in gs:
            f.write(struct.pack("<qq", len(txns), len(edges)))
            f.write(np.ascontiguousarray(txns).tobytes())
            f.write(np.ascontiguousarray(edges).tobytes())
    # the sanitizers' runtimes linked in statically: the program needs no place in anybody's preload list
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(HERE, "cycles_main.cpp"), os.path.join(CSRC, "cycles_host.cpp"),
                           os.path.join(CSRC, "graph_host.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "LC_CYCLE_MIN_WORK"}
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = []
    for ln in r.stdout.splitlines():
        f = ln.split()
        out.append((f[0], int(f[1]), dict(zip(f[2::2], (int(x) for x in f[3::2])))))
    return out


def test_reach_kats_under_the_sanitizers_give_the_library_s_counts(lines):
    cases = [rec for name, _, rec in lines if name == "reach"]
    assert len(cases) == len(KATS)
    for kat, rec in zip(KATS, cases):
        hit, s = abi.cycle_reach_host(*kat_arrays(kat), all_queries=True)
        _, early = abi.cycle_reach_host(*kat_arrays(kat))
        assert (rec["rc"], rec["rc_first"]) == (0, 0), kat["name"]
        assert (rec["first_hit"], rec["first_hit_early"], rec["hits"], rec["visited"], rec["visited_early"]) == \
            (s["first_hit"], early["first_hit"], int(hit.sum()), s["nodes_visited"], early["nodes_visited"]), kat["name"]
        assert (rec["first_hit"], rec["hits"], rec["visited"]) == (kat["first_hit"], sum(kat["hit"]), kat["nodes_visited"])


def test_graphs_under_the_sanitizers_give_the_library_s_counts(lines):
    cases = [rec for name, _, rec in lines if name == "graph"]
    gs = graphs()
    assert len(cases) == len(gs)
    asked = 0
    for (name, txns, edges), rec in zip(gs, cases):
        out, _ = abi.cycles_host(txns, edges)
        steps = out["steps"]
        assert (rec["rc"], rec["same"]) == (0, 1), name
        assert (rec["n_scc"], rec["scc"], rec["cls"], rec["steps"], rec["classes"]) == \
            (out["n_scc"], int(out["scc"].sum()), int(out["scc_class"].sum()),
             int((steps["txn"].astype(int) * 3 + steps["type"]).sum()),
             int((np.arange(1, 9) * out["n_class"]).sum())), name
        asked += rec["asked"]
    assert asked > 0  # (the hook was asked)


def test_generated_graphs_ran_and_met_every_kind(lines):
    gen = [rec for name, _, rec in lines if name == "gen-reach"]
    assert len(gen) == 7 and all(rec["rc"] == 0 and rec["first_hit"] == rec["first_hit_early"] for rec in gen)
    assert gen[0]["first_hit"] == -1 and any(rec["first_hit"] >= 0 for rec in gen)
    assert all(rec["visited_early"] <= rec["visited"] for rec in gen)
    gen = [rec for name, _, rec in lines if name == "gen-graph"]
    assert len(gen) == 9 and all((rec["rc"], rec["same"]) == (0, 1) for rec in gen)
    assert gen[0]["n_scc"] == 0 and any(rec["n_scc"] > 1 for rec in gen)
    assert gen[0]["asked"] == 0 and any(rec["asked"] > 0 for rec in gen)


def test_refusals(lines):
    refused = {name: (rec["rc"], rec["rc_first"]) for name, _, rec in lines
               if name in ("unsorted-queries", "pred-out-of-range", "head-is-source")}
    assert refused == {"unsorted-queries": (-22, -22), "pred-out-of-range": (-22, -22), "head-is-source": (-22, -22)}
