"""The engine's limb-sharded path — the native halves lf_cc_mult_evk_pre / _post, lf_switch_key_pre / _post, lf_ks_plan_fwd and the
three HIP graphs per (kind, level, lane, key, format knobs) of ckks_engine._sharded_segments — with one process per rank, all
ranks on the one GPU, on the edge parameter sets, edge words, the last levels, and under graph replay with NEW operands.

Every word is compared with the checker: ckks_engine(devices=["cpu"] * W, backend=OracleBackend(), **params), shard d of its
result against rank d's.  Operands come from tests/helpers.py (edge_ciphertext, edge_key, pre_rescale_ciphertext: words that follow
their limb's id, so a rank engine and the W-device checker see the same ones).  No tolerance anywhere.

  sets and worlds   WORLDS: (set, W) -> the levels tested: level 0, the first sharded level whose first digit owner differs from
                    level 0's (where one exists: sb40_K8 / sb45_K8 over 2 ranks have none, their two digit groups keep their
                    owners 1, 0 down to the level where rank 1 leaves), the last level with all W ranks alive, the last level
                    with 2 alive.  rule_levels() recomputes the table from the checker's own tables in every test.  The levels
                    where ONE rank is alive (rank 0 on the one-call entries, the others without rows) run the same ops behind the
                    sharded ones: the level bookkeeping.
  ops               cc_mult INTO the level (operands one level up; from level 0 into 1 for level 0) and, where there is one, out
                    of it; rotate_single by 1 and by -(N/2 - 1); conjugate; switch_key.  Patterns ("top", "top") and ("random",
                    "random") of test_engine_edges_gpu.PAIRS everywhere, every data pattern of ENGINE_EDGE_PATTERNS among the
                    replays, one pre_rescale_ciphertext product per level (0, round_at - 1, round_at, round_at + 1, q_drop - 1 in
                    the dropped row that travels from its owner; the owner is rank 1 or 2 at several of the levels).
  graph modes       graph_sharded False, then True: the capturing call, then replays with DIFFERENT operands, and between them
                    another level (whose segments get captured meanwhile), the other kind, a second key of the same kind, the
                    first key again.  EVERY result is compared.
  keys              one engine per point-to-point spawn runs with compact_key keys; a key is release_key'ed / invalidate_key'ed after its
                    segments were captured: the stale segments must be gone, a fresh key and the old one give the right words.
  which path ran    the five halves are counted with their `which` argument.  An eager op shows pre(3), one plan_fwd per run of
                    digits, post(3) — and, when it captures, exactly the launches of the three segments twice (warm-up + capture);
                    a replayed op shows pre(which=1) | switch_key_pre, then post(which=2), and NO plan_fwd; an sgraph entry
                    exists.  Ops off the sharded path (one rank alive; plain switch_key, which takes the step path) show none.
                    A quiet fall-back fails the count; the capture-failure warning of _sharded_segments is an error here.
  fence             sb41_K2 and sb40_K1 (W = 2, and solo; the point-to-point spawns): fresh engines under tests/helpers.Fence with the three FENCE_FILLS, refill()
                    before EVERY case — between a capture and its replays too, so a replay cannot lean on what the capturing op
                    left in scratch; after every case all guards whole, no output left at its fill, operands untouched, and
                    the words equal to the unfenced run's and the checker's.
  solo rank         the same with DistComm(solo_sharded=True) in a world of one (a child process: the pytest process never
                    initialises a process group), against the one-device checker.
  format knobs      sb41_K2 solo (mixed classes: lf_stack_planes answers 1): segments captured under the defaults, then
                    LF_TUNE_MORE_PLANES = 1, then LF_TUNE_DIGIT_PLANES = 0, then the defaults again: every result the checker's, and
                    no LF_ERR_STATE (the engine issued both halves).  The knobs are part of the segments' key.
  held streams      solo rank: op A on a stream held by the spin kernel (tests/helpers.hold), op B — whose replay shares ks_state /
                    ks_ext / ks_sum with A — on another: B's first launch does not complete inside the hold, both results right;
                    both ways round, and a replay directly behind an eager op of the other kind.  Captures come first: a capture
                    synchronises the device and would drain the hold.  With two ranks the gloo staging transport blocks the
                    host, so the ordering of the EXCHANGE against the graphs cannot be shown on one GPU: that stays with
                    tools/rccl_world1.py's stream_ordering.

Both forms of the exchange run the whole case list, except three ranks under the all-gather form: their first two levels and the
first level with one rank alive (the staged collective of three processes took 21 to 24 s with every level; the other levels run
under the point-to-point form).  The compact-key and the fenced engines run the first two levels and that tail level.

Limits: at most 3 ranks + the parent hold the GPU; every spawn runs under the process-group timeout, is joined with a deadline
and killed behind it; nothing is retried; every captured segment stays a single-stream linear capture."""
import datetime
import hashlib
import inspect
import json
import os
import socket
import sys
import tempfile
import time
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.helpers import (ENGINE_EDGE_PATTERNS, FENCE_FILLS, HALF_ENTRIES, BackendSpy, Fence, Untouched, edge_ciphertext, edge_key,
                           edge_param_sets, hold, independent_streams, pre_rescale_ciphertext, still_held)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = edge_param_sets()
# (set, W) -> the levels of rule_levels(); the ids of the tests carry them
WORLDS = {("sb40_K1", 2): (0, 1, 7), ("sb40_K1", 3): (0, 1, 6, 7), ("sb41_K2", 2): (0, 2, 3), ("sb41_K2", 3): (0, 1, 2, 3),
          ("sb40_K8", 2): (0, 7), ("sb45_K8", 2): (0, 7), ("sb20", 3): (0, 2, 3, 5)}
SOLO = {"sb41_K2": (0, 5), "sb40_K1": (0, 8)}
FENCED = ("sb41_K2", "sb40_K1")
HOLD_MS = 50              # tests/test_stream_contract_gpu.HOLD_MS
SPAWN_LIMIT_S = 300       # a whole spawn; the process group's own timeout is 120 s
F = ("plan_fwd", None)


# ---- the case list: plain data, the same for a rank and for the checker ------------------------------------------------------
def rule_levels(C, W, solo):
    nl = C.num_levels
    sharded = [lv for lv in range(nl) if solo or C.len_devices[lv] > 1]
    owner = lambda lv: C._ks_tables(lv)["groups"][0][0]
    out = {0, max(lv for lv in sharded if C.len_devices[lv] == W), max(sharded)}
    flipped = [lv for lv in sharded if owner(lv) != owner(0)]
    return tuple(sorted(out | set(flipped[:1])))


def script(levels, nl, alive, solo):
    """[case]: {"id", "grp": the tested level the case belongs to (the shorter runs pick by it), "op": mult | rot | conj | switch |
    release | invalidate, "level": the level of the op's plan (cc_mult: of its RESULT), "pat", "key", "seed", "pre", "graphs"}"""
    sharded = lambda lv: solo or alive[lv] > 1
    tail = [lv for lv in range(nl) if not sharded(lv)]
    tail = sorted({tail[0], tail[-1]}) if tail else []
    cases, seed = [], [0]

    def add(phase, grp, op, level, pat="", key="", pre=False, graphs=False):
        seed[0] += 1
        cases.append({"id": f"{phase}/{op}/L{level}/{pat}{'/pre' if pre else ''}/{key}/{seed[0]}", "grp": grp, "op": op, "level": level,
                      "pat": pat, "key": key, "seed": seed[0], "pre": pre, "graphs": graphs})

    for graphs, phase in ((False, "eager"), (True, "graph")):
        for i, L in enumerate(levels):
            into = max(L, 1)
            if not graphs:
                for pat, s in (("top", "A"), ("random", "B")):
                    add(phase, L, "mult", into, pat, "evk" + s)
                    if 1 <= L < nl - 1:
                        add(phase, L, "mult", L + 1, pat, "evk" + s)
                    add(phase, L, "rot", L, pat, "rot" + s)
                    add(phase, L, "conj", L, pat, "conj" + s)
                    add(phase, L, "switch", L, pat, "evk" + s)
                add(phase, L, "mult", into, "mixed", "evkA", pre=True)
                continue
            other = max(levels[(i + 1) % len(levels)], 1)
            g = lambda *a, **kw: add(phase, L, *a, graphs=True, **kw)
            g("mult", into, "top", "evkA")            # captures (unless an earlier level's `other` did)
            g("rot", L, "top", "rotA")                # captures
            g("mult", into, "random", "evkA")         # replay 1, new operands
            g("mult", other, "random", "evkA")        # another level in between
            g("rot", L, "random", "rotA")             # the other kind, replay 1
            g("mult", into, "top|0", "evkB")          # a second key of the kind: a second entry
            g("rot", L, "half", "rotB")
            g("mult", into, "mixed", "evkA", pre=True)   # the first key again, replay 2: the rounder's five values
            g("rot", L, "mixed", "rotA")              # replay 2
            g("conj", L, "top", "conjA")              # the switch kind under a third key
            g("mult", into, "half", "evkA")           # replay 3
            g("rot", L, "top|1", "rotA")              # replay 3
            g("conj", L, "random", "conjA")
            g("mult", into, "random", "evkB")
            g("switch", L, "top", "evkA")
        for L in tail:                                # one rank alive: behind the sharded levels, in both modes
            for pat, s in (("top", "A"), ("random", "B")):
                add(phase, L, "mult", L, pat, "evk" + s, graphs=graphs)
                add(phase, L, "rot", L, pat, "rot" + s, graphs=graphs)
                add(phase, L, "conj", L, pat, "conj" + s, graphs=graphs)
                add(phase, L, "switch", L, pat, "evk" + s, graphs=graphs)
            add(phase, L, "mult", L, "mixed", "evkA", pre=True, graphs=graphs)
    # a key dropped after its segments were captured, a fresh key, the old key again
    L = levels[0]
    r = lambda *a, **kw: add("rekey", L, *a, graphs=True, **kw)
    r("release", L, key="rotA")
    r("rot", L, "top", "rotC")
    r("rot", L, "top|0", "rotA")
    r("rot", L, "random", "rotA")
    r("invalidate", L, key="evkA")
    r("mult", max(L, 1), "top", "evkA")
    r("mult", max(L, 1), "random", "evkA")
    return cases


def variant_cases(cases, levels, variant, short):
    """the case list a variant runs: all of it for "plain" (unless `short`), else the cases of the first two tested levels and of
    the first level with one rank alive — levels pared, never patterns.  The rank and the parent both ask here."""
    if variant == "plain" and not short:
        return cases
    tails = sorted({c["grp"] for c in cases} - set(levels))
    keep = set(list(levels[:2]) + tails[:1])
    return [c for c in cases if c["grp"] in keep]


def make_keys(eng):
    N = eng.ctx.N
    rot1, rot2 = "rotation key:1", f"rotation key:{-(N // 2 - 1)}"
    return {"evkA": edge_key(eng, "top", 1), "evkB": edge_key(eng, "random", 2),
            "rotA": edge_key(eng, "top", 3, origin=rot1), "rotB": edge_key(eng, "random", 4, origin=rot2),
            "rotC": edge_key(eng, "random", 7, origin=rot1),
            "conjA": edge_key(eng, "top", 5, origin="conjugation key"), "conjB": edge_key(eng, "random", 6, origin="conjugation key")}


def operands(eng, c):
    L, pat, seed = c["level"], c["pat"], c["seed"]
    if c["op"] == "mult":
        if c["pre"]:
            return pre_rescale_ciphertext(eng, L - 1, pat, seed), pre_rescale_ciphertext(eng, L - 1, pat, seed + 5000, shift=1)
        return edge_ciphertext(eng, L - 1, pat, seed), edge_ciphertext(eng, L - 1, pat, seed + 5000)
    return (edge_ciphertext(eng, L, pat, seed),)


def run_case(eng, keys, c, ops):
    k = keys[c["key"]]
    if c["op"] == "mult":
        return eng.cc_mult(ops[0], ops[1], k)
    return {"rot": eng.rotate_single, "conj": eng.conjugate, "switch": eng.switch_key}[c["op"]](ops[0], k)


def digest(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return [list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]


def shard_digests(ct, d, multi):
    """the two components of device d's shard of a result (a rank engine holds one shard or none)"""
    out = []
    for comp in ct.data:
        i = 0 if multi else d
        out.append(digest(comp[i]) if i < len(comp) else None)
    return out


# ---- a rank -----------------------------------------------------------------------------------------------------------------
class HalfLog:
    """counts the five halves on a backend instance, with their `which`"""

    def __init__(self, be):
        self.log = []
        for name in HALF_ENTRIES:
            real = getattr(be, name)                    # (the fence's wrapper, where one is installed)
            sig = inspect.signature(getattr(type(be), name))

            def counted(*args, _real=real, _sig=sig, _name=name, **kw):
                b = _sig.bind(None, *args, **kw)
                b.apply_defaults()
                self.log.append((_name, b.arguments.get("which")))
                return _real(*args, **kw)

            setattr(be, name, counted)

    def take(self):
        got, self.log = self.log, []
        return got


def runs_of(eng, level, d):
    """(groups of digits this rank owns, maximal runs of foreign groups between them) at a level, from the level's tables"""
    own = foreign = 0
    inside = False
    for g in eng._ks_tables(level)["groups"]:
        if g[0] == d:
            own, inside = own + 1, False
        else:
            foreign, inside = foreign + (0 if inside else 1), True
    return own, foreign


def expected_halves(eng, c, rank, world, captured, knobs):
    """the half launches an op must show, and whether it leaves a new sgraph entry.  `captured`: the model of the engine's
    sgraph entries, {(kind, level, key name, format knobs)}."""
    L, op = c["level"], c["op"]
    on_path = (world == 1 or eng.len_devices[L] > 1) and rank < eng.len_devices[L] and op != "switch"
    if not on_path:
        return [], False
    kind = "mult" if op == "mult" else "switch"
    pre, post = ("cc_mult_pre", "cc_mult_post") if kind == "mult" else ("switch_key_pre", "switch_key_post")
    entry = (kind, L, c["key"], knobs)
    if c["graphs"] and entry in captured:
        return [(pre, 1 if kind == "mult" else None), (post, 2)], False
    own, foreign = runs_of(eng, L, rank)
    want = [(pre, 3 if kind == "mult" else None)] + [F] * (own + foreign) + [(post, 3)]
    if c["graphs"]:        # warm-up + capture of a1, a2, c
        want += ([("cc_mult_pre", 2)] * 2 if kind == "mult" else []) + [F] * (2 * own) + ([F] * foreign + [(post, 1)]) * 2
        captured.add(entry)
    return want, c["graphs"]


def sgraph_keys(eng):
    return [k for k in eng._tables if isinstance(k, tuple) and k and k[0] == "sgraph"]


def _rank(rank, world, port, outdir, cfg):
    cfg = json.loads(cfg)
    warnings.filterwarnings("ignore")
    warnings.filterwarnings("error", message="HIP-graph capture")          # a failed capture is a failed test, not a slower run
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    from tests import gloo_device_p2p
    gloo_device_p2p.install()
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine
    from liberate_fhe_amd.fhe.comm import DistComm
    params, solo = SETS[cfg["set"]], cfg["solo"]
    results = {}

    def engine():
        eng = ckks_engine(devices=["cuda:0"], comm=DistComm(local_device="cuda:0", exchange=cfg["exchange"], solo_sharded=solo), **params)
        assert eng._multi and eng.local_ids == [rank] and eng.backend.name.startswith("hip")
        return eng

    def knobs():
        return (lib.lf_tune(3, -1), lib.lf_tune(5, -1))

    late = []

    def one(eng, keys, c, log, captured, fence=None, ops=None, strict=True):
        """one case on a rank: the op, its half launches against the model, its sgraph entry, the fence; -> digests.
        strict=False: a launch count off the model goes into `late`, which the parent asserts empty AFTER it compared the
        words (the knob walk: wrong words are the finding, the counts say how the engine avoided them)."""
        if c["op"] in ("release", "invalidate"):
            key = keys[c["key"]]
            ptrs = {t.data_ptr() for t in eng._key_pack(key)}
            (eng.release_key if c["op"] == "release" else eng.invalidate_key)(key)
            stale = [k for k in sgraph_keys(eng) if k[5] in ptrs]
            assert not stale, (c["id"], "segments captured on a dropped pack are still held", stale)
            for e in [e for e in captured if e[2] == c["key"]]:
                captured.discard(e)
            return None
        eng.graph_sharded = c["graphs"]
        ops = operands(eng, c) if ops is None else ops
        keep = Untouched(ops=ops, key=keys[c["key"]]) if fence is not None else None
        if fence is not None:
            fence.refill()
            fence.never_written = []
        before = len(sgraph_keys(eng))
        log.take()
        res = run_case(eng, keys, c, ops)
        got = log.take()
        want, captures = expected_halves(eng, c, rank, world, captured, knobs())
        if not strict and (got != want or len(sgraph_keys(eng)) != before + (1 if captures else 0)):
            late.append([c["id"], "half launches", got, "expected", want, "sgraph entries", before, len(sgraph_keys(eng))])
        elif strict:
            assert got == want, (c["id"], rank, "half launches", got, "expected", want)
            assert len(sgraph_keys(eng)) == before + (1 if captures else 0), (c["id"], rank, "sgraph entries", before, len(sgraph_keys(eng)))
        if fence is not None:
            torch.cuda.synchronize()
            fence.check()
            assert not fence.never_written, (c["id"], "outputs left at their fill", fence.never_written)
            keep.check(c["id"])
        return shard_digests(res, rank, True)

    if cfg["mode"] == "edges":
        for variant in cfg["variants"]:
            eng = engine()
            nl = eng.num_levels
            cases = script(cfg["levels"], nl, list(eng.len_devices[:nl]), solo)
            cases = variant_cases(cases, cfg["levels"], variant, cfg.get("short"))
            fence = Fence(eng, FENCE_FILLS[variant]) if variant in FENCE_FILLS else None
            log = HalfLog(eng.backend)
            keys = make_keys(eng)
            if variant == "compact":
                assert sum(eng.compact_key(k) for k in keys.values()) > 0
            captured = set()
            for c in cases:
                got = one(eng, keys, c, log, captured, fence)
                if got is not None:
                    results[f"{variant}|{c['id']}"] = got
            if any(c["graphs"] and c["op"] in ("mult", "rot", "conj") and rank < eng.len_devices[c["level"]]
                   and (solo or eng.len_devices[c["level"]] > 1) for c in cases):
                assert captured and sgraph_keys(eng), "no segment was captured"
            del eng, keys, fence, log
            torch.cuda.synchronize()
    elif cfg["mode"] == "knobs":
        eng = engine()
        log, keys, captured = HalfLog(eng.backend), make_keys(eng), set()
        plan = eng._op_plan(1, 0)[0]
        assert knobs() == (1, 3) and lib.lf_stack_planes(eng.ctx.logN, plan.ell, plan.q_host) == 1
        try:
            for c in knob_cases():
                if c["op"] == "tune":
                    lib.lf_tune(c["which"], c["value"])
                    continue
                got = one(eng, keys, c, log, captured, strict=False)     # (HipError LF_ERR_STATE would end the rank here)
                results[f"plain|{c['id']}"] = got
        finally:
            lib.lf_tune(3, 1)
            lib.lf_tune(5, 3)
        if len(captured) != 6 or len(sgraph_keys(eng)) != 6:            # two kinds under three settings; the defaults' reused
            late.append(["sgraph entries at the end", len(captured), len(sgraph_keys(eng))])
        results["_late"] = late
    elif cfg["mode"] == "streams":
        eng = engine()
        log, keys, captured = HalfLog(eng.backend), make_keys(eng), set()
        warm, held = stream_cases()
        for c in warm:
            results[f"plain|{c['id']}"] = one(eng, keys, c, log, captured)
        torch.cuda.synchronize()
        s1, s2 = independent_streams("cuda:0")
        launchers = BackendSpy(eng.backend).launchers()
        first = {}

        def watch(name):
            real = getattr(eng.backend, name)

            def watched(*a, **kw):
                ret = real(*a, **kw)
                if first.get("armed") and "ev" not in first:      # right behind B's first launch, on B's stream
                    first["ev"], first["name"] = torch.cuda.Event(), name
                    first["ev"].record(torch.cuda.current_stream())
                return ret
            setattr(eng.backend, name, watched)
        for name in launchers:
            watch(name)
        for a_case, b_case in held:
            ops_a, ops_b = operands(eng, a_case), operands(eng, b_case)
            torch.cuda.synchronize()
            first.clear()
            log.take()
            ev = hold(s1, HOLD_MS)
            t0 = time.perf_counter()
            with torch.cuda.stream(s1):
                eng.graph_sharded = a_case["graphs"]
                res_a = run_case(eng, keys, a_case, ops_a)
            halves_a = log.take()
            first["armed"] = True
            with torch.cuda.stream(s2):
                eng.graph_sharded = b_case["graphs"]
                res_b = run_case(eng, keys, b_case, ops_b)
            first["armed"] = False
            halves_b = log.take()
            enqueue_ms = 1e3 * (time.perf_counter() - t0)
            while not first["ev"].query() and time.perf_counter() - t0 < HOLD_MS / 2e3:
                pass
            finished, on = first["ev"].query(), still_held(ev)
            host_ms = 1e3 * (time.perf_counter() - t0)
            torch.cuda.synchronize()
            tag = (a_case["id"], b_case["id"], first["name"], round(enqueue_ms, 2), round(host_ms, 2))
            assert on, ("the hold ran out before the check: nothing shown", tag)
            assert not finished, ("B's first launch completed while A's stream was held", tag)
            for c, got in ((a_case, halves_a), (b_case, halves_b)):
                want, _ = expected_halves(eng, c, rank, world, set(captured), knobs())
                assert got == want, (c["id"], "half launches", got, want)
            results[f"plain|{a_case['id']}"] = shard_digests(res_a, rank, True)
            results[f"plain|{b_case['id']}"] = shard_digests(res_b, rank, True)
    else:
        raise ValueError(cfg["mode"])
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(results, f)
    dist.barrier()
    dist.destroy_process_group()


def _case(op, level, pat, key, seed, graphs=True, pre=False, tag="k"):
    return {"id": f"{tag}/{op}/L{level}/{pat}/{key}/{seed}", "grp": level, "op": op, "level": level, "pat": pat, "key": key,
            "seed": seed, "pre": pre, "graphs": graphs}


def knob_cases():
    """defaults (capture, replay) | MORE_PLANES = 1: the operand stack raw | DIGIT_PLANES = 0: the digits raw | defaults again"""
    out, seed = [], 100
    for which, value in ((None, None), (5, 1), (3, 0), ("restore", None)):
        if which == "restore":
            out += [{"op": "tune", "which": 3, "value": 1}, {"op": "tune", "which": 5, "value": 3}]
        elif which is not None:
            out.append({"op": "tune", "which": which, "value": value})
        for rep, (pm, pr) in enumerate((("top", "random"), ("random", "top"))):
            seed += 2
            out.append(_case("mult", 1, pm, "evkA", seed, pre=rep == 1, tag=f"k{which}{value}"))
            out.append(_case("rot", 0, pr, "rotA", seed + 1, tag=f"k{which}{value}"))
    return out


def stream_cases():
    warm = [_case(op, lv, pat, key, 200 + i, tag="warm") for i, (op, lv, pat, key) in enumerate(
        (("mult", 1, "top", "evkA"), ("rot", 1, "top", "rotA"), ("mult", 1, "random", "evkA"), ("rot", 1, "random", "rotA")))]
    held = [(_case("mult", 1, "mixed", "evkA", 210, tag="heldA"), _case("rot", 1, "half", "rotA", 211, tag="B")),
            (_case("rot", 1, "top|0", "rotA", 212, tag="heldA"), _case("mult", 1, "top|1", "evkA", 213, tag="B")),
            (_case("rot", 1, "random", "rotA", 214, graphs=False, tag="heldA-eager"), _case("mult", 1, "half", "evkA", 215, tag="B")),
            (_case("mult", 1, "random", "evkA", 216, graphs=False, tag="heldA-eager"), _case("rot", 1, "mixed", "rotA", 217, tag="B"))]
    return warm, held


# ---- the parent -------------------------------------------------------------------------------------------------------------
_CHECKER = {}


def checker(name, W):
    """(checker engine, its keys, {case key: per-device digests}) of a (set, world), built once per process"""
    if (name, W) not in _CHECKER:
        from liberate_fhe_amd.fhe import ckks_engine
        from tests.oracle_backend import OracleBackend
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            C = ckks_engine(devices=["cpu"] * W, backend=OracleBackend(), **SETS[name])
        _CHECKER[name, W] = (C, make_keys(C), {})
    return _CHECKER[name, W]


def want_digests(name, W, c):
    C, keys, memo = checker(name, W)
    k = (c["op"], c["level"], c["pat"], c["key"], c["seed"], c["pre"])
    if k not in memo:
        res = run_case(C, keys, c, operands(C, c))
        memo[k] = [shard_digests(res, d, False) for d in range(W)]
    return memo[k]


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn(world, cfg):
    """the ranks of one configuration, joined under a deadline; -> {rank: {variant|case id: digests}}"""
    with tempfile.TemporaryDirectory() as outdir:
        ctx = mp.start_processes(_rank, args=(world, free_port(), outdir, json.dumps(cfg)), nprocs=world, join=False, start_method="spawn")
        deadline = time.monotonic() + SPAWN_LIMIT_S
        while not ctx.join(timeout=2):              # (a rank that raised ends its peers and raises here)
            if time.monotonic() > deadline:
                for p in ctx.processes:
                    p.kill()
                raise AssertionError(f"the ranks of {cfg} were still running after {SPAWN_LIMIT_S} s: killed")
        return {r: json.load(open(os.path.join(outdir, f"rank{r}.json"))) for r in range(world)}


def compare(name, W, cases_of, got):
    """cases_of: {variant: the case list the ranks were to run under it}.  Every (variant, case) must have been reported by every
    rank — a case a rank left out fails here, it is not passed over — and every shard must be the checker's."""
    bad, n = [], 0
    for variant, cases in cases_of.items():
        ops = [c for c in cases if c["op"] not in ("release", "invalidate", "tune")]
        missing = [(f"{variant}|{c['id']}", r) for c in ops for r in range(W) if f"{variant}|{c['id']}" not in got[r]]
        assert not missing, f"{len(missing)} (case, rank) results were not reported: {missing[:6]}"
        extra = sorted(set(k for r in range(W) for k in got[r] if k.startswith(variant + "|")) - {f"{variant}|{c['id']}" for c in ops})
        assert not extra, f"results of cases that are not on the list of {variant}: {extra[:6]}"
        for c in ops:
            key = f"{variant}|{c['id']}"
            want = want_digests(name, W, c)
            for r in range(W):
                n += 1
                if got[r][key] != want[r]:
                    bad.append((key, r, got[r][key], want[r]))
    assert not bad, f"{len(bad)} of {n} shards differ from the checker's: {bad[:6]}"
    return n


def edge_run(name, W, levels, exchange, solo):
    C = checker(name, W)[0]
    assert rule_levels(C, W, solo) == tuple(levels), (rule_levels(C, W, solo), levels)
    # the whole case list under both forms of the exchange; the runs that differ from it in the keys' storage and in what the
    # scratch holds — neither meets the exchange's form — under the point-to-point one only
    variants = ["plain"] + (["compact"] + (sorted(FENCE_FILLS) if name in FENCED and W <= 2 else []) if exchange == "p2p" else [])
    # three ranks under the all-gather form (21 to 24 s with every level on an MI355X: the staged collective of three processes is
    # what takes the time): the first two levels and the first level with one rank alive; every level under the point-to-point form
    short = exchange == "allgather" and W == 3
    cfg = {"mode": "edges", "set": name, "exchange": exchange, "solo": solo, "levels": list(levels), "variants": variants, "short": short}
    got = spawn(W, cfg)
    nl = C.num_levels
    cases = script(list(levels), nl, list(C.len_devices[:nl]), solo)
    cases_of = {v: variant_cases(cases, list(levels), v, short) for v in variants}
    compare(name, W, cases_of, got)
    if short:
        levels = levels[:2]
    plain = [c for c in cases_of["plain"] if c["op"] not in ("release", "invalidate")]
    for v in variants[1:]:
        assert len(cases_of[v]) >= 30, (v, "too few cases")
    # every data pattern and every op under replay, the rounder's product at every level
    assert {c["pat"] for c in plain if c["graphs"]} >= set(ENGINE_EDGE_PATTERNS)
    assert {c["level"] for c in plain if c["pre"]} >= {max(lv, 1) for lv in levels}


WORLD_IDS = [f"{n}-W{w}-L{'.'.join(map(str, lv))}" for (n, w), lv in WORLDS.items()]


@pytest.mark.parametrize("exchange", ["p2p", "allgather"])
@pytest.mark.parametrize("world", list(WORLDS), ids=WORLD_IDS)
def test_ranks_on_one_gpu_equal_the_checker_on_edge_words_eager_and_replayed(world, exchange):
    """Where the owner of the dropped row is not rank 0: sb40_K1 over 2 ranks into level 2 (rank 1) and over 3 ranks into
    levels 1 and 7 (rank 2), sb41_K2 into level 3 (rank 1), sb20 into level 3 (rank 2), sb40_K8 / sb45_K8 everywhere
    (rank 1)."""
    name, W = world
    edge_run(name, W, WORLDS[world], exchange, solo=False)


@pytest.mark.parametrize("exchange", ["p2p", "allgather"])
@pytest.mark.parametrize("name", list(SOLO), ids=[f"{n}-solo-L{'.'.join(map(str, lv))}" for n, lv in SOLO.items()])
def test_a_solo_rank_on_the_sharded_path_equals_the_one_device_checker(name, exchange):
    edge_run(name, 1, SOLO[name], exchange, solo=True)


def test_format_knobs_flipped_between_replays_give_the_checkers_words():
    """ADVICE.md (round 6): the sgraph key held no lf_tune state and a replay bypasses the host-side LF_ERR_STATE guard, so an
    eager pre(which=1) under a flipped LF_TUNE_MORE_PLANES wrote a raw operand stack that the replayed a1 read as planes:
    silently wrong words.  The two format knobs are part of the key now: the first op under a new setting runs eagerly and
    captures, the defaults' segments are found again afterwards (the counts in the rank assert both)."""
    cfg = {"mode": "knobs", "set": "sb41_K2", "exchange": "p2p", "solo": True}
    got = spawn(1, cfg)
    cases = knob_cases()
    late = got[0].pop("_late")
    assert compare("sb41_K2", 1, {"plain": cases}, got) == 16
    assert not late, late[:4]


def test_held_streams_on_the_sharded_path_order_replays_behind_the_lanes_last_op():
    cfg = {"mode": "streams", "set": "sb41_K2", "exchange": "p2p", "solo": True}
    got = spawn(1, cfg)
    warm, held = stream_cases()
    cases = warm + [c for pair in held for c in pair]
    assert compare("sb41_K2", 1, {"plain": cases}, got) == 12
