"""The engine's stream contract, tested with HELD streams (ckks_engine._ws, _same_stream, _run_groups, _prepare_ks, _key_pack):

  * the scratch of an engine belongs to the engine and its lane, not to a stream: an op that arrives on another current stream
    than the lane's previous op first makes its stream wait for that op — alternating streams is safe and serial;
  * ops of DIFFERENT engines are independent;
  * the batched methods fork a side lane and join it before they return, and every lazily built piece of shared state the side
    lane reads (key pack, per-level tables, fp64 twiddle twins) is built on the caller's stream before the fork;
  * a device tensor the engine drops (a replaced workspace, an evicted table, a key's planes copy, a compacted raw pack) is not
    handed out again while work the engine enqueued on another stream still uses it.

A test that enqueues ops back to back on idle streams passes whenever the kernels happen not to overlap.  Here a stream is kept
busy for HOLD_MS by the project's one-wave spin kernel (tests/helpers.hold), so that "B waited for A" is two event queries:

    ev = hold(s1); A on s1; B on s2; done recorded on s2      ->  not done.query() and still_held(ev)

Both true: B waits for something behind the hold.  If the hold ran out first the check says nothing, and the test FAILS with the
host time it measured (no inconclusive case is allowed).  The two streams are shown to run independently on this process's
hardware queues first (tests/helpers.independent_streams): on a shared queue every such check would pass whatever the engine does.

  A  every public op, both ways round beside cc_mult, on the native path (logN 13) and the orchestrated one (logN 12); the set of
     native entries the cases reach is the backend's whole set, so an op added later without a case fails here.
  B  a host-side spy, no timing: the wait_stream comes BEFORE the op's first backend call.
  C  two engines: B of engine 2 completes while A of engine 1 is held — the documented independence, and the proof that the
     harness sees an op that does not wait.
  D  the callers of _run_groups on a fresh engine with fresh keys over zeroed free memory: the main lane or the side lane held
     at its first launch behind the fork, or the caller's stream held right before the fork event is recorded.
  E  the sites where the engine drops device memory: the reader held, the free triggered from another stream, the freed size
     allocated and zero-filled on the stream the block belongs to.

All words are torch.equal to the same call on one stream with nothing held.  Operands: liberate_fhe_amd.utils.synth.

The sharded halves and their graph-replayed segments (_sharded_segments) are held in a solo-rank child process by
tests/test_sharded_edges_gpu.py (a replay behind a held replay and behind a held eager op of the other kind, both ways round).
Not covered: the ordering of two ranks' EXCHANGE against the graphs on device streams (the gloo staging transport of a one-GPU box
blocks the host; tools/rccl_world1.py's stream_ordering is what there is), the in-process engine over two logical devices,
ntt_cuda's per-stream workspace (tests/test_ntt_cuda_gpu.py), the samplers' generator state under two streams."""
import time
import warnings

import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests import test_fenced_ops_gpu as F
from tests.helpers import NATIVE_ENTRIES, BackendSpy, hold, independent_streams, still_held, zeroed_free_memory
from tests.test_pc_matmul_gpu import layer_of

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)

DEV = "cuda:0"
LT13 = dict(logN=13, num_scales=5, num_special_primes=2, is_secured=False)      # tests/test_lt_matmul_batch_gpu.LT
LT12 = dict(LT13, logN=12)                                                       # the orchestrated path
# LAB_NOTES.md "Held streams": ten times the slowest warmed enqueue among the cases of A (both ops of a check), not below 20 ms
HOLD_MS = 50
LV = 0
_ENG, _OPS, _WANT = {}, {}, {}


def engine(name):
    """"main13" / "second13" (the native path), "main12" (orchestrated), "drops13" (section E): built once per process and kept"""
    if name not in _ENG:
        from liberate_fhe_amd.fhe import ckks_engine
        _ENG[name] = ckks_engine(devices=[DEV], **(LT12 if name.endswith("12") else LT13))
    return _ENG[name]


def ops(name):
    """the operands of a ring degree (tests/test_fenced_ops_gpu.Ops): made once, by the main engine of that degree"""
    name = "main12" if name.endswith("12") else "main13"
    if name not in _OPS:
        _OPS[name] = F.Ops(engine(name))
    return _OPS[name]


def foreign(x):
    """a copy of a key with tensors of its own: a key the engine has not made (its pack is the engine's copy: _key_pack)"""
    if isinstance(x, torch.Tensor):
        return x.clone()
    if hasattr(x, "origin") and hasattr(x, "_replace"):
        return x._replace(data=foreign(x.data))
    if isinstance(x, (list, tuple)):
        return type(x)(foreign(v) for v in x)
    return x


# ---- the cases: (id, f(engine, ops) -> result, the native entries it reaches at logN 13) -------------------------------------
STEPS, BSTEPS, N1 = (0, 1, 2), (0, 1, 2, 3), 2
TWO = [[(0, 1), (2,)], [(1, 2), (0,)]]
TWO_BSGS = [[(0, 1, 2), (3,)], [(1, 2), (0,)]]
POLY = (0.25, 0.5, -0.125, 0.0625)


def _pairs(o, k=2):
    return [(o.ct(50 + i, LV), o.ct(51 + i, LV)) for i in range(k)]


def _galois_key(e, o):
    return e._new([o.key(1), o.key(2)], "galois key", include_special=True, ntt_state=True, montgomery_state=True)


def _ltm(e, o, kind):
    W, cts, keys = F.layer(o, LV, TWO_BSGS if kind == "bsgs" else TWO, N1 if kind == "bsgs" else None)
    if kind == "batch":
        return e.lt_matmul_batch(W, [cts, cts[::-1], cts], keys)
    return e.lt_matmul_bsgs(W, cts, keys) if kind == "bsgs" else e.lt_matmul(W, cts, keys)


def _pc_batch(e, o):
    W, cts, bias = layer_of(F.pc_pool(o, LV), 2, 2)
    return e.pc_matmul_batch(W, [cts, cts[::-1], cts], bias)


def _matmul(e, o, n):
    a, b, c = o.cts(3, LV)
    if n == 1:
        return e.cc_matmul([[a]], [[b]], o.evk())
    return e.cc_matmul([[a, b], [b, c]], [[b, c], [c, a]], o.evk())


def _inner_keys(e, o):
    return o.keys(e.inner_sum_steps(4, 1, 2))


A_OP = ("cc_mult", lambda e, o: e.cc_mult(o.ct(50, LV), o.ct(51, LV), o.evk()), {"cc_mult_evk"})
CASES = [
    A_OP,
    ("cc_mult_then_relinearize", lambda e, o: e.relinearize(e.cc_mult(o.ct(50, LV), o.ct(51, LV), o.evk(), relin=False), o.evk()), set()),
    ("rescale", lambda e, o: e.rescale(o.ct(50, LV)), set()),
    ("rotate_single", lambda e, o: e.rotate_single(o.ct(50, LV), o.key(1)), {"switch_key_native"}),
    ("conjugate", lambda e, o: e.conjugate(o.ct(50, LV), o.key(3)), {"switch_key_native"}),
    ("rotate_galois", lambda e, o: e.rotate_galois(o.ct(50, LV), _galois_key(e, o), 3), {"switch_key_native"}),
    ("rotate_hoisted", lambda e, o: e.rotate_hoisted(o.ct(50, LV), [o.key(1), o.key(2)]), {"rotate_hoisted_native"}),
    ("linear_transform", lambda e, o: e.linear_transform(o.ct(50, LV), o.diags(7, LV, STEPS), o.keys(STEPS)), {"linear_transform_native"}),
    ("linear_transform_bsgs", lambda e, o: e.linear_transform(o.ct(50, LV), o.diags(9, LV, BSTEPS, N1), o.keys(BSTEPS)),
     {"linear_transform_bsgs_native"}),
    ("linear_transform_batch", lambda e, o: e.linear_transform_batch(o.cts(3, LV), o.diags(7, LV, STEPS), o.keys(STEPS)),
     {"linear_transform_batch_native", "linear_transform_native"}),
    ("linear_transform_batch_bsgs", lambda e, o: e.linear_transform_batch(o.cts(3, LV), o.diags(9, LV, BSTEPS, N1), o.keys(BSTEPS)),
     {"linear_transform_bsgs_batch_native", "linear_transform_bsgs_native"}),
    ("cc_dot", lambda e, o: e.cc_dot(_pairs(o), o.evk()), {"cc_dot_native"}),
    ("cc_dot_batch", lambda e, o: e.cc_dot_batch([_pairs(o), _pairs(o)[:1], _pairs(o)[1:]], o.evk()), {"cc_dot_batch_native", "cc_dot_native"}),
    ("cc_matmul", lambda e, o: _matmul(e, o, 2), {"cc_matmul_native"}),
    ("weighted_sums", lambda e, o: e.weighted_sums(o.cts(2, LV), [[0.5, -0.25], [1.0, 0.125]], [0.1, -0.2]), {"weighted_sums_native"}),
    ("poly_eval", lambda e, o: e.poly_eval(o.ct(50, LV), POLY, o.evk()), {"weighted_sums_native", "cc_mult_evk", "cc_dot_native"}),
    ("poly_eval_batch", lambda e, o: e.poly_eval_batch(o.cts(3, LV), POLY, o.evk()),
     {"weighted_sums_native", "cc_mult_evk_batch_native", "cc_mult_evk", "cc_dot_batch_native", "cc_dot_native"}),
    ("pc_mult", lambda e, o: e.pc_mult(o.pt(40, LV), o.ct(50, LV)), set()),
    ("pc_add", lambda e, o: e.pc_add(o.pt(60, LV, "add"), o.ct(50, LV)), set()),
    ("pc_dot", lambda e, o: e.pc_dot([(o.pt(40, LV), o.ct(50, LV)), (o.pt(41, LV), o.ct(51, LV))], o.pt(60, LV + 1, "add")), {"pc_dot_native"}),
    ("pc_matmul", lambda e, o: e.pc_matmul(*layer_of(F.pc_pool(o, LV), 2, 2)), {"pc_matmul_native"}),
    ("pc_matmul_batch", _pc_batch, {"pc_matmul_batch_native", "pc_matmul_native"}),
    ("lt_matmul", lambda e, o: _ltm(e, o, "flat"), {"lt_matmul_native"}),
    ("lt_matmul_bsgs", lambda e, o: _ltm(e, o, "bsgs"), {"lt_matmul_bsgs_native"}),
    ("lt_matmul_batch", lambda e, o: _ltm(e, o, "batch"), {"lt_matmul_batch_native", "lt_matmul_native"}),
    ("rotate_sum", lambda e, o: e.rotate_sum(o.ct(50, LV), [o.key(1), o.key(2)]), {"rotate_sum_native"}),
    ("inner_sum", lambda e, o: e.inner_sum(o.ct(50, LV), 4, _inner_keys(e, o), radix=2), {"rotate_sum_native"}),
    ("rotate_sum_batch", lambda e, o: e.rotate_sum_batch(o.cts(3, LV), [o.key(1), o.key(2)]), {"rotate_sum_batch_native", "rotate_sum_native"}),
    ("inner_sum_batch", lambda e, o: e.inner_sum_batch(o.cts(3, LV), 4, _inner_keys(e, o), radix=2), {"rotate_sum_batch_native", "rotate_sum_native"}),
    ("cc_mult_batch", lambda e, o: e.cc_mult_batch(_pairs(o, 3), o.evk()), {"cc_mult_evk_batch_native", "cc_mult_evk"}),
    ("rotate_single_batch", lambda e, o: e.rotate_single_batch(o.cts(3, LV), o.key(1)), {"switch_key_batch_native", "switch_key_native"}),
]
CASE = {c[0]: c for c in CASES}
IDS = [c[0] for c in CASES]
RINGS = ("main13", "main12")


def native_seen(spy):
    return {n for n in spy.calls() if n in NATIVE_ENTRIES}


def want(ring, name):
    """the words of a case on one stream (the default one) with nothing held, computed once; it also warms the op.  The native
    entries are counted here: a quiet fall-back to the orchestration fails instead of passing."""
    if (ring, name) not in _WANT:
        e, o = engine(ring), ops(ring)
        _, f, entries = CASE[name]
        with BackendSpy(e.backend) as spy:
            words = F.flat_words(f(e, o))
        torch.cuda.synchronize()
        seen = native_seen(spy)
        if ring.endswith("12"):
            assert not seen, (name, seen)
        else:
            assert seen == entries, (name, sorted(seen))
        _WANT[ring, name] = ([w.clone() for w in words], seen)
    return _WANT[ring, name][0]


def streams():
    return independent_streams(DEV)


def ordered(ev, done, t0, what):
    """the ordering check: `done` (recorded behind B) has not happened, and the hold is still on.  Asked half a hold after it
    began: an instant after the enqueue no kernel of B could have completed, waited or not (section C is the control: there
    the same poll sees B complete)."""
    enqueue_ms = 1e3 * (time.perf_counter() - t0)
    while not done.query() and time.perf_counter() - t0 < HOLD_MS / 2e3:
        pass
    finished = done.query()
    held = still_held(ev)
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert held, (f"{what}: inconclusive — the host took {enqueue_ms:.1f} ms to enqueue, the hold of {HOLD_MS} ms ran out before "
                  f"the check at {host_ms:.1f} ms")
    assert not finished, f"{what}: B completed while A's stream was held ({host_ms:.1f} ms after the hold began): it did not wait"


# ---- A: every op is ordered behind the lane's previous op ---------------------------------------------------------------------
@pytest.mark.parametrize("first", ["cc_mult_first", "op_first"])
@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("ring", RINGS)
def test_an_op_on_another_stream_waits_for_the_lanes_previous_op(ring, name, first):
    e, o = engine(ring), ops(ring)
    s1, s2 = streams()
    names = ("cc_mult", name) if first == "cc_mult_first" else (name, "cc_mult")
    wants = [want(ring, n) for n in names]
    fa, fb = CASE[names[0]][1], CASE[names[1]][1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        ra = fa(e, o)
    with torch.cuda.stream(s2):
        rb = fb(e, o)
    done = torch.cuda.Event()
    done.record(s2)
    ordered(ev, done, t0, f"{ring}: {names[0]} held on s1, then {names[1]} on s2")
    torch.cuda.synchronize()
    F.assert_same(F.flat_words(ra), wants[0], f"{ring} {names[0]} (A, held)")
    F.assert_same(F.flat_words(rb), wants[1], f"{ring} {names[1]} (B, behind it)")


def test_the_cases_reach_every_native_entry_of_the_backend():
    """An op added later without a case above fails here: the entries the cases reach are the backend's `*_native` methods plus
    cc_mult_evk (tests/helpers.NATIVE_ENTRIES is the same list, held to the backend by the first assertion)."""
    be = engine("main13").backend
    entries = {n for n in dir(type(be)) if n.endswith("_native")} | {"cc_mult_evk"}
    assert entries == set(NATIVE_ENTRIES), sorted(entries ^ set(NATIVE_ENTRIES))
    seen = set()
    for name in IDS:
        want("main13", name)
        seen |= _WANT["main13", name][1]
    assert seen == entries, f"no case reaches {sorted(entries - seen)}; unknown entries {sorted(seen - entries)}"


# ---- B: the wait comes before the first launch --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("ring", RINGS)
def test_the_wait_comes_before_the_ops_first_backend_call(ring, name):
    """No timing: the op runs on s2 after cc_mult on s1 under a spy on every launching method of the backend, on the public
    entries of engine.ntt.ops (the element-wise kernels the orchestrated path, pc_add and pc_mult launch through) and on
    torch.cuda.Stream.wait_stream.  An op that launches on its operands, or reads engine state, and orders itself afterwards
    passes the ordering check (its last event still waits) and fails here.  The limit: plain torch ops (a clone, an index copy)
    are not seen — for an op that launches nothing else before its wait the test only says that a wait exists."""
    e, o = engine(ring), ops(ring)
    s1, s2 = streams()
    w = want(ring, name)
    want(ring, "cc_mult")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        A_OP[1](e, o)
    with BackendSpy(e.backend, also=[e.ntt.ops]) as spy:
        with torch.cuda.stream(s2):
            r = CASE[name][1](e, o)
    waits = [i for i, x in enumerate(spy.log) if x == ("wait", s2.cuda_stream, s1.cuda_stream)]
    calls = [i for i, x in enumerate(spy.log) if x[0] == "call"]
    assert waits, f"{ring} {name}: no s2.wait_stream(s1) at all; log {spy.log[:6]}"
    assert not calls or waits[0] < calls[0], f"{ring} {name}: {spy.log[calls[0]][1]} ran before the wait; log {spy.log[:waits[0] + 1]}"
    torch.cuda.synchronize()
    F.assert_same(F.flat_words(r), w, f"{ring} {name}")


# ---- C: different engines are independent (and the harness sees an op that does not wait) --------------------------------------
@pytest.mark.parametrize("name", ["cc_mult", "rotate_single", "linear_transform", "pc_dot"])
def test_an_op_of_another_engine_does_not_wait(name):
    """A of engine 1 held on s1, B of engine 2 on s2: B completes while the hold is on (polled for at most HOLD_MS / 2)."""
    e1, e2, o = engine("main13"), engine("second13"), ops("main13")
    s1, s2 = streams()
    want("main13", "cc_mult")
    f = CASE[name][1]
    w = F.flat_words(f(e2, o))
    w = [t.clone() for t in w]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        ra = A_OP[1](e1, o)
    with torch.cuda.stream(s2):
        rb = f(e2, o)
    done = torch.cuda.Event()
    done.record(s2)
    while not done.query() and still_held(ev) and time.perf_counter() - t0 < HOLD_MS / 2e3:
        pass
    finished, held = done.query(), still_held(ev)
    ms = 1e3 * (time.perf_counter() - t0)
    assert held, f"{name}: inconclusive — the hold of {HOLD_MS} ms ran out after {ms:.1f} ms"
    assert finished, f"{name} of engine 2 had not completed {ms:.1f} ms into engine 1's hold: the engines are not independent"
    torch.cuda.synchronize()
    F.assert_same(F.flat_words(rb), w, f"{name} of engine 2")
    F.assert_same(F.flat_words(ra), want("main13", "cc_mult"), "cc_mult of engine 1")


# ---- D: lanes — fork, prepare, join -------------------------------------------------------------------------------------------
def _batch_cc_mult(e, cts, key):
    return e.cc_mult_batch([(cts[i], cts[i + 1]) for i in range(len(cts) - 1)], key)


def _loop_cc_mult(e, cts, key):
    return [e.cc_mult(cts[i], cts[i + 1], key) for i in range(len(cts) - 1)]


def _dots(cts):
    return [[(cts[i], cts[i + 1]), (cts[i + 1], cts[i])][:1 + i % 2] for i in range(len(cts) - 1)]


LANE_OPS = {
    "cc_mult_batch": ("evk", _batch_cc_mult, _loop_cc_mult),
    "rotate_single_batch": ("rotk", lambda e, cts, key: e.rotate_single_batch(cts[:-1], key),
                            lambda e, cts, key: [e.rotate_single(ct, key) for ct in cts[:-1]]),
    "cc_dot_batch": ("evk", lambda e, cts, key: e.cc_dot_batch(_dots(cts), key),
                     lambda e, cts, key: [e.cc_dot(p, key) for p in _dots(cts)]),
}


def _fresh_key(e, ref, kind, own):
    if own:       # made by the engine: the own-pack path of _key_pack (the key's tensors are views of the raw pack)
        sk = e.create_secret_key()
        return e.create_evk(sk) if kind == "evk" else e.create_rotation_key(sk, 1)
    # (synth registers a key with the engine it is made for, as that engine's own: a copy is a key no engine has seen)
    return foreign(synth.key_switch_key(ref, 77) if kind == "evk" else synth.key_switch_key(ref, 101, origin="rotation key:1"))


@pytest.mark.parametrize("held,own,members", [("main", False, 6), ("main", True, 6), ("main", False, 7), ("side", False, 6), ("caller", False, 6)])
@pytest.mark.parametrize("op", sorted(LANE_OPS))
def test_lanes_fork_prepare_and_join(op, held, own, members):
    """A caller of _run_groups on a fresh engine with a fresh key over zeroed free memory, no op run before: `members` members
    (6: a group of 4 on lane 0 and one of 2 on lane 1; 7: a second job on lane 0).  The side lane runs on the stream the file has
    shown to be independent of the caller's.
      main    lane 0 is held at its first launch behind the fork: whatever lane 1 reads that lane 0's job would build lazily is
              read unbuilt; lane 1 must complete while the hold is on (it depends on nothing behind the fork).
      side    lane 1 is held at its first launch: an event on the caller's stream right behind the call passes the ordering
              check — the join.
      caller  the caller's stream is held right behind `prepare` (whose table builds block the host on that stream: held any
              earlier, the host would sit out the hold there), before _run_groups records the fork event: an event on the side
              stream behind the call passes the ordering check — the fork carries the hold to the side lane."""
    from liberate_fhe_amd.fhe import ckks_engine
    kind, batch, loop = LANE_OPS[op]
    s1, s2 = streams()
    ref = engine("second13")
    cts = [synth.ciphertext(ref, 300 + i, LV) for i in range(members + 1)]
    torch.cuda.synchronize()
    zeroed_free_memory(DEV, 1 << 28)
    e = ckks_engine(devices=[DEV], **LT13)
    e._lane_streams[0] = [s2]                   # the engine would create one of its own: this one is known to be independent
    key = _fresh_key(e, ref, kind, own)
    torch.cuda.synchronize()
    state = {"armed": False, "ev": None, "t0": None}
    real_prepare = e._prepare_ks

    def prepare(*args):
        real_prepare(*args)
        state["armed"] = True                   # _run_groups forks right behind it
        if held == "caller" and state["ev"] is None:
            state["t0"] = time.perf_counter()
            state["ev"] = hold(torch.cuda.current_stream(), HOLD_MS)

    def before(name):
        if state["armed"] and state["ev"] is None and held != "caller" and e._lane == (0 if held == "main" else 1):
            state["ev"] = hold(torch.cuda.current_stream(), HOLD_MS)

    e._prepare_ks = prepare
    t0 = time.perf_counter()
    with BackendSpy(e.backend, before=before):
        with torch.cuda.stream(s1):
            got = batch(e, cts, key)
    ev = state["ev"]
    assert ev is not None, f"{op}: lane {held} launched nothing behind the fork"
    on_caller, on_side = torch.cuda.Event(), torch.cuda.Event()
    on_caller.record(s1)
    on_side.record(s2)
    what = f"{op}, {held} held, {'own' if own else 'foreign'} key, {members} members"
    if held == "side":
        ordered(ev, on_caller, t0, what + ": the caller's stream behind the call (join)")
    elif held == "caller":
        ordered(ev, on_side, state["t0"], what + ": the side lane behind the call (fork)")
    else:
        while not on_side.query() and still_held(ev) and time.perf_counter() - t0 < HOLD_MS / 2e3:
            pass
        finished, still = on_side.query(), still_held(ev)
        ms = 1e3 * (time.perf_counter() - t0)
        assert still, f"{what}: inconclusive — the hold of {HOLD_MS} ms ran out after {ms:.1f} ms"
        assert finished, f"{what}: the side lane had not completed {ms:.1f} ms into the main lane's hold"
    torch.cuda.synchronize()
    w = loop(ref, cts, foreign(key) if own else key)
    F.assert_same(F.flat_words(got), F.flat_words(w), what)


# ---- E: memory freed under pending work ---------------------------------------------------------------------------------------
def refill(nbytes, ev, what, copies=4):
    """`copies` tensors of `nbytes` allocated and zero-filled on the CURRENT stream — the one the freed block belongs to, so the
    allocator hands it out again — while the hold `ev` is on: the fills must COMPLETE inside the hold, or the test says nothing."""
    fills = [torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV) for _ in range(copies)]
    filled = torch.cuda.Event()
    filled.record()
    t0 = time.perf_counter()
    while not filled.query() and still_held(ev) and time.perf_counter() - t0 < HOLD_MS / 2e3:
        pass
    assert filled.query() and still_held(ev), f"{what}: inconclusive — the fills had not completed inside the hold of {HOLD_MS} ms"
    return fills


def untouched(fills, what):
    """a tensor the caller allocated after the engine dropped a block must not be written by the engine's pending work"""
    for i, f in enumerate(fills):
        assert not bool(f.any()), f"{what}: fill {i}, allocated after the free, was written by the engine ({int((f != 0).sum())} words)"


def _nbytes(ts):
    return max(t.untyped_storage().nbytes() for t in ts)


def test_compact_key_under_a_held_stream_keeps_the_raw_pack_until_the_planes_are_built():
    """compact_key on never-used keys made on the default stream, called under s1 while s1 is held: the planes build waits on s1
    and reads the raw pack, whose storage compact_key frees at once — back to the DEFAULT stream's pool, where the zero fills take
    it while the build is still pending."""
    e, ref, o = engine("drops13"), engine("second13"), ops("main13")
    s1, _ = streams()
    sk = e.create_secret_key()
    evk, rotk = e.create_evk(sk), e.create_rotation_key(sk, 1)
    a, b = o.ct(50, LV), o.ct(51, LV)
    w = [ref.cc_mult(a, b, foreign(evk)), ref.rotate_single(a, foreign(rotk))]
    nbytes = _nbytes(e._key_packs[id(e._key_anchor(evk))]["packs"])
    torch.cuda.synchronize()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        assert e.compact_key(evk) > 0 and e.compact_key(rotk) > 0
    fills = refill(nbytes, ev, "compact_key")
    with torch.cuda.stream(s1):
        got = [e.cc_mult(a, b, evk), e.rotate_single(a, rotk)]
    torch.cuda.synchronize()
    F.assert_same(F.flat_words(got), F.flat_words(w), "cc_mult and rotate_single under keys compacted on a held stream")
    untouched(fills, "compact_key")


def test_cc_matmul_growing_its_store_keeps_the_old_one_until_its_reader_is_done():
    """The store of cc_matmul is allocated by a 1 x 1 x 1 product on the default stream; the same product is held on s1; a
    2 x 2 x 2 product on s2 replaces the store with a larger one.  The old block goes back to the default stream's pool while
    the held product has yet to use it as scratch: what is allocated there next would be written by it."""
    e, ref, o = engine("drops13"), engine("second13"), ops("main13")
    s1, s2 = streams()
    key = ("matmul_ws", 0, 0)
    e._workspace.pop(key, None)
    w = [ref.cc_matmul([[o.ct(50, LV)]], [[o.ct(51, LV)]], o.evk()), _matmul(ref, o, 2)]
    e.cc_matmul([[o.ct(50, LV)]], [[o.ct(51, LV)]], o.evk())
    _matmul(e, o, 2)
    e._workspace.pop(key)                       # warmed (plans, key pack); the store itself starts small again
    torch.cuda.synchronize()
    e.cc_matmul([[o.ct(50, LV)]], [[o.ct(51, LV)]], o.evk())
    small = e._workspace[key]
    nbytes, ptr = small.untyped_storage().nbytes(), small.data_ptr()
    del small
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        r1 = e.cc_matmul([[o.ct(50, LV)]], [[o.ct(51, LV)]], o.evk())
    with torch.cuda.stream(s2):
        r2 = _matmul(e, o, 2)
    assert e._workspace[key].data_ptr() != ptr and e._workspace[key].numel() * 8 > nbytes
    fills = refill(nbytes, ev, "cc_matmul")
    done = torch.cuda.Event()
    done.record(s2)
    ordered(ev, done, t0, "cc_matmul 2 x 2 x 2 behind the held 1 x 1 x 1")
    torch.cuda.synchronize()
    F.assert_same(F.flat_words([r1, r2]), F.flat_words(w), "cc_matmul, the store replaced under a pending call")
    untouched(fills, "cc_matmul")


def test_weighted_sums_evicting_a_table_under_two_streams():
    """NOT a held-stream test: 65 distinct weight rows cycle through the 64 tables of weighted_sums, alternating between s1 and
    s2, so that every call misses, builds its table and evicts the least recently used one; the words are pinned.  A reader of
    the evicted table cannot be held: an eviction only follows a table build, a host-blocking copy on a stream that is ordered
    behind the lane's earlier ops, so the host never reaches it while a reader of that lane is pending, and a hit makes its table
    the youngest (LAB_NOTES.md "Held streams").  s1 is held all the same, and the premise is asserted: the first build drains the
    hold.  Should a build stop blocking the host, that assertion fails and says what this test then has to become."""
    e, ref, o = engine("drops13"), engine("second13"), ops("main13")
    s1, s2 = streams()
    cts = o.cts(2, LV)
    rows = [[[i + 1, 3 - i]] for i in range(65)]
    w = [ref._weighted_sums_int(cts, r) for r in rows]
    for r in rows:
        e._weighted_sums_int(cts, r)
    torch.cuda.synchronize()
    got = []
    ev = hold(s1, HOLD_MS)
    for i in range(2 * 65):
        if i == 1:      # the first miss has built its table behind the hold: the host was kept until the hold had run out
            assert not still_held(ev), "a table build no longer blocks the host: rewrite this test with the evicted table's reader held"
        with torch.cuda.stream(s1 if i % 2 == 0 else s2):
            got.append(e._weighted_sums_int(cts, rows[i % 65]))
        fill = torch.zeros(4096, dtype=torch.int64, device=DEV)      # (on the default stream: the tables' pool)
    torch.cuda.synchronize()
    assert len(e._wsum_tables) == 64 and not bool(fill.any())
    F.assert_same(F.flat_words(got), F.flat_words(w + w), "weighted_sums with every call evicting a table")


def test_release_key_of_a_foreign_key_keeps_its_pack_until_the_pending_rotation_has_read_it():
    e, ref, o = engine("drops13"), engine("second13"), ops("main13")
    s1, s2 = streams()
    fk = foreign(o.key(1))
    a = o.ct(50, LV)
    w = ref.rotate_single(a, fk)
    e.rotate_single(a, fk)                      # the engine's copy of the key, made on the default stream
    nbytes = _nbytes(e._key_packs[id(e._key_anchor(fk))]["packs"])
    torch.cuda.synchronize()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        r = e.rotate_single(a, fk)
    with torch.cuda.stream(s2):
        e.release_key(fk)
    assert id(e._key_anchor(fk)) not in e._key_packs
    fills = refill(nbytes, ev, "release_key")
    torch.cuda.synchronize()
    F.assert_same(F.flat_words(r), F.flat_words(w), "rotate_single pending while its foreign key is released")
    untouched(fills, "release_key")


def test_a_key_edited_in_place_keeps_its_old_planes_until_the_pending_rotation_has_read_them():
    """An own key edited in place (the version counter moves, the words do not): the next use rebuilds the planes copy and
    drops the old one, which the rotation held on s1 has yet to read."""
    e, ref, o = engine("drops13"), engine("second13"), ops("main13")
    s1, s2 = streams()
    k = synth.key_switch_key(e, 101, origin="rotation key:1")       # (registered as the engine's own: views of one raw pack)
    a = o.ct(50, LV)
    w = ref.rotate_single(a, foreign(k))
    e.rotate_single(a, k)                       # the planes copy, made on the default stream
    hit = e._key_packs[id(e._key_anchor(k))]
    assert hit["own"] and hit.get("planes")
    nbytes, ptr = _nbytes(hit["planes"]), hit["planes"][0].data_ptr()
    torch.cuda.synchronize()
    ev = hold(s1, HOLD_MS)
    with torch.cuda.stream(s1):
        r1 = e.rotate_single(a, k)
    with torch.cuda.stream(s2):
        e._key_anchor(k).add_(0)
        r2 = e.rotate_single(a, k)
    assert hit["planes"][0].data_ptr() != ptr
    fills = refill(nbytes, ev, "planes rebuilt")
    torch.cuda.synchronize()
    F.assert_same(F.flat_words([r1, r2]), F.flat_words([w, w]), "rotate_single around an in-place edit of its key")
    untouched(fills, "planes rebuilt")
