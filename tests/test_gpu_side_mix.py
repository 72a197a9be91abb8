"""The side checkers interleaved on one context: lc_set_full, lc_append_check,
lc_wr_check and lc_watch_check in turn and again in reverse order, each on
its first known-answer history, then one lc_check.  Each checker keeps a
state of one shape (an arena, pinned words, events) made by its first call;
every output array and count must equal its host twin's whatever ran in
between."""
import pytest

import test_gpu_append as GA
import test_gpu_setfull as GS
import test_gpu_watch as GW
import test_gpu_wr as GR
from helpers import load_kats, pack_keys
from jepsen.etcd_amd import abi, append as AP, setfull as SF, watch as W, wr as WR

pytestmark = pytest.mark.gpu


def test_side_checkers_interleaved_on_one_context():
    sf, ap, wr, wt = GS.KATS[0], GA.KATS[0], GR.KATS[0], GW.KATS[0]
    sf_enc, ap_enc, wr_enc = SF.encode(sf["history"]), AP.encode(ap["history"]), WR.encode(wr["history"])
    wt_enc = W.encode(wt["history"], wt["concurrency"])
    verdict = {1: True, 0: False, -1: "unknown"}

    def set_full(ctx, what):
        _, gs = GS._agree(ctx, sf_enc.adds, sf_enc.reads, sf_enc.values, sf["linearizable"], what)
        assert verdict[gs["valid"]] == sf["valid"], what

    def append(ctx, what):
        _, gs = GA._agree(ctx, ap_enc.txns, ap_enc.mops, ap_enc.values, what)
        assert verdict[gs["valid"]] == ap["valid"], what

    def wr_check(ctx, what):
        _, gs = GR._agree(ctx, wr_enc.txns, wr_enc.mops, True, what)
        assert verdict[gs["valid"]] == wr["valid"], what

    def watch(ctx, what):
        GW.agree_arrays(ctx, wt_enc.threads, wt_enc.values, nn=len(wt_enc.nonmonotonic), what=what)

    calls = (set_full, append, wr_check, watch)
    kat = load_kats()[0]
    ops, off = pack_keys([kat["ops"]])
    with abi.Context(device_mask=1) as ctx:
        for call in calls + calls[::-1]:
            call(ctx, call.__name__)
        rc, r = ctx.check(ops, off)
        assert rc == 0
        assert r["verdict"][0] == (1 if kat["valid"] else 0)
        assert r["fail_op"][0] == kat["fail_op"]
        assert r["fail_prefix_end"][0] == kat["fail_prefix_end"]
