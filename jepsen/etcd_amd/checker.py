"""Checker mirror of the reference's plugin boundary for the register workload.

The reference builds, at /root/reference/src/jepsen/etcd/register.clj:108-112,

    (independent/checker
      (checker/compose {:linear   (checker/linearizable {:model (->VersionedRegister 0 nil)})
                        :timeline (timeline/html)}))

and jepsen calls it through the jepsen.checker/Checker protocol,
(check [this test history opts]) -> {:valid? ...}.  `register_checker()` is
the drop-in for that whole expression: one object whose check() splits the
history by key, completes and packs it on the host, and decides every key in
one batched GPU call (include/lincheck.h).  The result has
jepsen.independent/checker's shape:

    {"valid?": merged, "results": {k: {...}}, "failures": [k ...]}

with merged = false > "unknown" > true, and "failures" the keys whose
:valid? is false (jepsen.independent keeps :unknown keys out of :failures,
since :unknown is truthy in Clojure).  Each key's map has checker/compose's
shape, {"valid?", "linear": <the GPU verdict>, "timeline": ...}; with
timeline_dir set, the timeline half renders <dir>/independent/<k>/
timeline.html on the host (timeline.py), as jepsen's timeline/html would.
An invalid key's map also carries knossos's diagnostics (diagnostics.py):
"previous-ok", "configs" and "final-paths" — from the search's own frontier
just before the failing return (up to 10 configurations: one batched device
search over every invalid key, lc_check_frontiers; one more over the counted
search, lc_check_frontiers_counted, for the keys with more than 64 ops open,
whose pending lists it returns whole; and lc_fx_frontier for a key neither
takes), and "last-op" from the witness of the prefix
before the failing return (lc_aux) for keys the version-order and gap tiers
decided.

Errors: a key with malformed records is "unknown" alone (cause
"malformed"), as jepsen.independent would lose only that key; unusable
arguments raise LcError, and jepsen's check-safe turns an exception into
{:valid? :unknown :error ...}, which `check_safe` reproduces.
"""
import os

import numpy as np

from . import abi, diagnostics as D, events as E, history as H, linear_svg as LS, timeline as TL, \
    witness as W

UNKNOWN = "unknown"
# an invalid key the batched device search (lc_check_frontiers) could not
# take, and which the version-order / gap tiers decided, is re-searched alone
# (lc_fx_frontier) for knossos's :configs only when it has at most this many
# crashed ops (the frontier of a version-pinned key grows with its crashed ops
# only)
FRONTIER_MAX_CRASHED = 16
CERT_KINDS = {0: "none", 1: "dup", 2: "unreach", 3: "claims", 4: "pair", 5: "order", 6: "hall",
              7: "proof"}


class VersionedRegister:
    """The model of register.clj:55-96 as data: its initial state.  The step
    function itself runs on the GPU (check_kernel.hip, `legal`)."""

    def __init__(self, version=0, value=None):
        self.version = version
        self.value = value

    name = "versioned-register"

    def __repr__(self):  # register.clj:57
        return "v%s: %s" % (self.version, self.value)


class CASRegister:
    """knossos.model/cas-register: a value, read/write/cas, no versions."""
    name = "cas-register"
    version = 0

    def __init__(self, value=None):
        self.value = value


class Register(CASRegister):
    """knossos.model/register: read/write only (a :cas is :unknown)."""
    name = "register"


class Mutex:
    """knossos.model/mutex, the lock workload's model (lock.clj:244):
    :acquire / :release of one lock, initially free."""
    name = "mutex"
    version = 0
    value = None


def _merge_valid(vs):
    vs = list(vs)
    if any(v is False for v in vs):
        return False
    if any(v == UNKNOWN for v in vs):
        return UNKNOWN
    return True


class RegisterChecker:
    """Drop-in for independent/checker + checker/linearizable(VersionedRegister)
    (register.clj:108-112).  With independent=False it is a plain
    checker/linearizable over the whole history, e.g. the lock workload's
    (checker/linearizable {:model (model/mutex)}) at lock.clj:243-244; the
    result is then one key's map (no :results)."""

    def __init__(self, model=None, device_mask=0, max_configs_per_key=0, independent=True,
                 timeline_dir=None, time_budget_ms=0, whole_gpu=True, frontier_max_keys=1000,
                 counted_classes=True, search_witness=False, counted_witness=True,
                 device_split=False):
        self.model = model or VersionedRegister(0, None)
        # the per-key split and the history completion on the device
        # (lc_check_events): check() writes one event record per op map
        # (events.encode) and rebuilds the completed ops from the records the
        # device packed.  A history events cannot express (events.Unsupported)
        # takes the host path; split_fallbacks counts those calls.  Value ids
        # are then the whole history's, not per key
        self.device_split = device_split
        self.split_fallbacks = 0
        # cap on the frontier re-searches one check() runs for diagnostics of
        # witnessed invalid keys (each is one key's search up to its failing
        # return, bounded by max_configs_per_key / time_budget_ms); 0: none
        self.frontier_max_keys = frontier_max_keys
        self.device_mask = device_mask
        self.max_configs_per_key = max_configs_per_key
        self.independent = independent
        self.timeline_dir = timeline_dir
        self.time_budget_ms = time_budget_ms
        # a key one workgroup's search leaves :unknown at the configuration
        # budget is searched again over the whole GPU (LC_FLAG_WHOLE_GPU):
        # knossos keeps searching until it runs out of memory or time, so the
        # drop-in does too by default (time_budget_ms bounds it)
        self.whole_gpu = whole_gpu
        # a key the tiers leave :unknown because more than 64 ops were open at
        # once is searched again with its crashed writes/CAS counted per class
        # (LC_FLAG_COUNTED_CLASSES), one wavefront per key inside the same
        # call, before the whole-GPU re-search: the same results, 21x
        # sooner for keys that hold one configuration (mutex histories) and
        # 1.1x for frontiers of a few thousand; keys with frontiers of tens
        # of thousands are quicker with counted_classes=False
        self.counted_classes = counted_classes
        # a key a search tier decided (every version-less model's keys) gets
        # no witness from the tiers; with search_witness the same call searches
        # each such key once more, depth first, for a linearization
        # (LC_FLAG_SEARCH_WITNESS), and its map gains "linearization" (its
        # ops in that order) and "witness-certified" (the order checked
        # against the definition on the host, witness.certify); an invalid
        # key's "last-op" then comes from the order's last op
        self.search_witness = search_witness
        # ... and a key that search leaves because more than 64 ops are open
        # at once (the crash-heavy keys the counted tier decides) is searched
        # once more with its crashed writes/CAS counted per class
        # (LC_FLAG_COUNTED_WITNESS): the same two entries for those keys.
        # Means something only with search_witness.
        self.counted_witness = counted_witness
        self._ctx = None
        self._fx = None

    def _flags(self):
        """lc_opts.flags of this checker's calls."""
        return (abi.LC_FLAG_WHOLE_GPU if self.whole_gpu else 0) | \
            (abi.LC_FLAG_COUNTED_CLASSES if self.counted_classes else 0) | \
            (abi.LC_FLAG_SEARCH_WITNESS if self.search_witness else 0) | \
            (abi.LC_FLAG_COUNTED_WITNESS if self.search_witness and self.counted_witness else 0)

    def _context(self):
        if self._ctx is None:
            self._ctx = abi.Context(self.device_mask)
        return self._ctx

    def _frontier(self):
        if self._fx is None:
            from .fx import FrontierExchange
            dev = 0
            while self.device_mask and not (self.device_mask >> dev) & 1:
                dev += 1
            self._fx = FrontierExchange(device=dev)
        return self._fx

    def _check_split_on_device(self, history, o):
        """The front half of check() through lc_check_events: what H.pack and
        the check16 / check32 call return, rebuilt from the device's records.
        None when the history cannot be written as events."""
        m = self.model
        try:
            ev, keys, table, index = E.encode(history, m.name, self.independent, m.value)
        except E.Unsupported:
            self.split_fallbacks += 1
            return None
        if not keys:
            return [], None, None, None, None, None
        _, res, wit, kind, cert, cset, (ops32, key_off, key_base, completion) = \
            self._context().check_events(ev, len(keys), o, witness=True, certificate=True, packed=True)
        # positions -> the history's own indices
        base = np.repeat(key_base, np.diff(key_off))
        call = ops32[:, 4].astype(np.uint32).astype(np.int64) + base
        ret32 = ops32[:, 5].astype(np.uint32).astype(np.int64)
        crashed = ret32 == abi.LC_INF32
        ret = np.where(crashed, 0, ret32 + base)
        ops = np.zeros((len(ops32), 6), dtype=np.int64)
        ops[:, :4] = ops32[:, :4]
        ops[:, 4] = index[call]
        ops[:, 5] = np.where(crashed, abi.LC_INF, index[ret])
        res = res.copy()
        failed = res["fail_prefix_end"] >= 0
        res["fail_prefix_end"][failed] = index[res["fail_prefix_end"][failed]]

        def op_at(pos):  # the op map as split_by_key hands it on
            op = dict(history[pos])
            op.setdefault("index", int(index[pos]))
            if self.independent:
                op["value"] = op["value"].value
            return op

        done = []
        for i in range(len(keys)):
            d = []
            for r in range(int(key_off[i]), int(key_off[i + 1])):
                inv = op_at(int(call[r]))
                comp = op_at(int(completion[r])) if completion[r] >= 0 else None
                ok = not crashed[r]
                d.append({"f": H._kw(inv.get("f")), "value": comp.get("value") if ok else inv.get("value"),
                          "call": int(ops[r, 4]), "ret": int(ops[r, 5]), "invoke": inv,
                          "completion": comp, "type": "ok" if ok else "info"})
            done.append(d)
        return keys, ops, key_off, done, [table] * len(keys), (res, wit, kind, cert, cset)

    def check(self, test, history, opts=None):
        m = self.model
        # the initial value is interned first in every key (id 0); the mutex
        # starts free (id MUTEX_FREE)
        init = H.MUTEX_FREE if m.name == "mutex" else (0 if m.value is not None else H.LC_NIL)
        o = abi.default_opts(self.max_configs_per_key, m.version, init, flags=self._flags(),
                             time_budget_ms=self.time_budget_ms)
        split = self._check_split_on_device(history, o) if self.device_split else None
        if split is not None:
            keys, ops, key_off, done, values, checked = split
        else:
            checked = None
            values = []
            keys, ops, key_off, done = H.pack(history, model=m.name, independent=self.independent,
                                              init_value=m.value, values_out=values)
        if not keys:
            return {"valid?": True, "results": {}, "failures": []}
        # the drop-in's call (ABI 5): 16-byte records when every value id
        # fits 15 bits, else 24-byte ones — what crosses PCIe (the JVM shim
        # packs them directly; here lc_pack16 / lc_pack32 narrow the 48-byte
        # pack by the same rules)
        p16 = abi.pack16(ops, key_off) if checked is None else None
        if checked is not None:
            res, wit, kind, cert, cset = checked
        elif p16 is not None:
            ops16, key_base = p16
            _, res, wit, kind, cert, cset = self._context().check16(
                ops16, key_off, key_base, o, witness=True, certificate=True)
        else:
            ops32, key_base = abi.pack32(ops, key_off)
            _, res, wit, kind, cert, cset = self._context().check32(
                ops32, key_off, key_base, o, witness=True, certificate=True)
        witnessed_keys = kind == abi.LC_WITNESS_PREFIX if m.name == "versioned-register" \
            else [False] * len(keys)
        cfg_errors = {}
        cfgs_of = self._configs(ops, key_off, res, o, witnessed_keys, cfg_errors)
        results = {}
        n_fallback = 0  # one-key frontier re-searches run for diagnostics in this call
        for i, k in enumerate(keys):
            r = res[i]
            v = {1: True, 0: False}.get(int(r["verdict"]), UNKNOWN)
            out = {"valid?": v, "analyzer": "mi355x",
                   "configs-explored": int(r["configs_explored"]),
                   "max-frontier": int(r["max_frontier"])}
            if v is False:
                d = done[i][int(r["fail_op"])]
                out["op"] = d["completion"] or d["invoke"]
                out["fail-prefix-end"] = int(r["fail_prefix_end"])
                # why the prefix at the failing return has no linearization
                # (include/lincheck.h LC_CERT_*; checkable from the records)
                ck = CERT_KINDS.get(int(cert[i][0]), "none")
                out["certificate"] = {"kind": ck}
                if ck in ("dup", "unreach", "claims", "pair", "order"):
                    out["certificate"]["ops"] = [done[i][int(x)]["completion"] or done[i][int(x)]["invoke"]
                                                 for x in cert[i][1:3] if x >= 0]
                elif ck == "hall":
                    out["certificate"]["positions"] = [
                        int(x) for x in cset[key_off[i]:key_off[i] + int(cert[i][3])]]
                elif ck == "proof":  # the case splits: (position, cases) in preorder
                    out["certificate"]["splits"] = [
                        ((int(x) & 0xFFFFFFFF) >> 15 & 0x7FFF, int(x) & 0x7FFF)
                        for x in cset[key_off[i]:key_off[i] + int(cert[i][3])]]
                recs = ops[key_off[i]:key_off[i + 1]]
                witnessed = m.name == "versioned-register" and kind[i] == abi.LC_WITNESS_PREFIX
                # knossos's :configs are its search's frontier just before the
                # failing return: every invalid key's came from one batched
                # device search (lc_check_frontiers, _configs), or for a key
                # with more than 64 ops open from one more over the counted
                # search (lc_check_frontiers_counted); a key neither could
                # take is re-searched alone by the frontier exchange
                # (lc_fx_frontier, which lists at most 64 pending ops)
                # — any key the search decided, and witnessed keys with at
                # most FRONTIER_MAX_CRASHED crashed ops — at most
                # frontier_max_keys such re-searches per call (the Clojure
                # shim counts the same way); beyond that, or if the re-search
                # fails, the witness's one configuration (with
                # "configs-error" saying why)
                cfgs, err = cfgs_of.get(i), cfg_errors.get(i)
                if cfgs is None and n_fallback < self.frontier_max_keys and (
                        not witnessed or
                        int((recs[:, 5] == abi.LC_INF).sum()) <= FRONTIER_MAX_CRASHED):
                    n_fallback += 1
                    try:
                        cfgs = self._frontier().frontier(recs, int(r["fail_op"]), D.MAX_ENTRIES, o)
                    except Exception as e:  # noqa: BLE001 — diagnostics only; the verdict stands
                        err = repr(e)
                wa = D.invalid_analysis(done[i], int(r["fail_op"]), int(r["fail_prefix_end"]),
                                        wit[key_off[i]:key_off[i + 1]],
                                        init=(m.version, m.value)) if witnessed else None
                if cfgs is not None:
                    out.update(D.frontier_analysis(
                        done[i], int(r["fail_op"]), int(r["fail_prefix_end"]), cfgs, values[i],
                        versioned=m.name == "versioned-register"))
                    if wa is not None and "last-op" in wa:
                        out["last-op"] = wa["last-op"]  # the witness's last linearized op
                elif wa is not None:
                    out.update(wa)
                else:
                    out["previous-ok"] = D.previous_ok(done[i], int(r["fail_prefix_end"]))
                if err is not None:
                    out["configs-error"] = err
            if self.search_witness and kind[i] in (abi.LC_WITNESS_ORDER_FULL,
                                                   abi.LC_WITNESS_ORDER_PREFIX):
                recs = ops[key_off[i]:key_off[i + 1]]
                w = wit[key_off[i]:key_off[i + 1]]
                lin = [done[i][j]["completion"] or done[i][j]["invoke"] for j in W.order(recs, w)]
                out["linearization"] = lin
                out["witness-certified"] = W.certify(recs, w, int(kind[i]),
                                                     cut=int(r["fail_prefix_end"]) - 1,
                                                     init=(m.version, init))
                if v is False and lin and "last-op" not in out:
                    out["last-op"] = lin[-1]
            if v == UNKNOWN:
                # the Clojure shim's keys (mi355x.clj): :cause and :error
                cause = abi.REASONS.get(int(r["reason"]), int(r["reason"]))
                out["cause"] = cause
                out["error"] = ["lincheck-reason", cause]
            results[k] = out
        if not self.independent:
            return results[None]
        subs = H.split_by_key(H.index_history(history)) if self.timeline_dir else None
        for i, (k, lin) in enumerate(results.items()):
            if self.timeline_dir and lin["valid?"] is False and "final-paths" in lin:
                # jepsen's checker/linearizable renders a failed analysis
                # into the key's directory as linear.svg
                lin["linear-svg"] = LS.write(
                    os.path.join(self.timeline_dir, "independent", str(k), "linear.svg"),
                    done[i], lin, title="key %s" % (k,))
            results[k] = self._composed(k, lin, subs)
        return {"valid?": _merge_valid(r["valid?"] for r in results.values()),
                "results": results,
                "failures": [k for k, r in results.items() if r["valid?"] is False]}

    def _configs(self, ops, key_off, res, opts, witnessed=None, errors=None):
        """knossos's :configs of every invalid key in one device call
        (lc_check_frontiers), and of the keys it left out — more than 64 ops
        open — in one more over the counted search
        (lc_check_frontiers_counted): {key index: [(version, value id,
        pending)]}, the keys neither search could take left out.  The second
        call takes the keys the one-key fallback would take (`witnessed`:
        bool per key; a witnessed key only with at most FRONTIER_MAX_CRASHED
        crashed ops); if it fails, they get its error in `errors` and fall
        back as before."""
        import numpy as np
        inv = np.nonzero(res["verdict"] == abi.LC_INVALID)[0]
        if self.frontier_max_keys <= 0 or len(inv) == 0:
            return {}

        def sub(idx):
            parts = [ops[key_off[i]:key_off[i + 1]] for i in idx]
            sub_off = np.zeros(len(idx) + 1, dtype=np.int64)
            sub_off[1:] = np.cumsum([len(x) for x in parts])
            return np.concatenate(parts), sub_off

        try:
            got = self._context().check_frontiers(*sub(inv), res["fail_op"][inv], D.MAX_ENTRIES, opts)
        except Exception:  # noqa: BLE001 — diagnostics only; the verdicts stand
            # (as mi355x.clj batched-configs): every key falls back to the
            # one-key re-search or its witness
            return {}
        out = {int(i): c for i, c in zip(inv, got) if c is not None}
        rest = [int(i) for i in inv if int(i) not in out and (
            witnessed is None or not witnessed[i] or
            int((ops[key_off[i]:key_off[i + 1], 5] == abi.LC_INF).sum()) <= FRONTIER_MAX_CRASHED)]
        if rest:
            try:
                got, _ = self._context().check_frontiers_counted(
                    *sub(rest), res["fail_op"][rest], D.MAX_ENTRIES, opts)
                out.update({i: c for i, c in zip(rest, got) if c is not None})
            except abi.LcError as e:
                if errors is not None:
                    errors.update({i: repr(e) for i in rest})
        return out

    def _composed(self, k, linear, subs):
        """checker/compose's per-key map (register.clj:109-112)."""
        if subs is None:
            return {"valid?": linear["valid?"], "linear": linear}
        path = os.path.join(self.timeline_dir, "independent", str(k), "timeline.html")
        tl = TL.write(path, subs[k], title="key %s" % (k,),
                      cex_index=linear.get("fail-prefix-end"))
        return {"valid?": _merge_valid([linear["valid?"], tl["valid?"]]),
                "linear": linear, "timeline": tl}

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        if self._fx is not None:
            self._fx.close()
            self._fx = None


def register_checker(**kw):
    return RegisterChecker(**kw)


def linearizable(model, **kw):
    """checker/linearizable {:model model} over the whole history (no
    independent split)."""
    return RegisterChecker(model=model, independent=False, **kw)


def check_safe(checker, test, history, opts=None):
    """jepsen.checker/check-safe: exceptions become {:valid? :unknown :error}."""
    try:
        return checker.check(test, history, opts)
    except Exception as e:  # noqa: BLE001 — mirrors check-safe's catch-all
        return {"valid?": UNKNOWN, "error": repr(e)}
