"""tests/helpers.Fence without a GPU: on a checker engine the fenced run of two ops leaves the plain run's words and intact guards
(the fence costs nothing when all is well), and against a stub backend entry every fault the fence exists for is reported, at the
right buffer, side and offset: a word before an output, behind an output, behind the workspace, in a plan scratch guard, a modified
operand, an output the entry never wrote."""
import pytest
import torch

from liberate_fhe_amd.utils import synth
from tests.helpers import FENCE_FILLS, HALF_ENTRIES, NATIVE_ENTRIES, Fence, FenceError, Untouched

SMALL = dict(logN=12, num_scales=3, num_special_primes=2, is_secured=False)


def engine(stub=None, **attrs):
    """a fresh checker engine; stub: {entry name: function} set on its backend before the fence wraps it"""
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.oracle_backend import OracleBackend
    be = OracleBackend()
    for name, fn in {**(stub or {}), **attrs}.items():
        setattr(be, name, fn)
    return ckks_engine(devices=["cpu"], backend=be, **SMALL)


def words(ct):
    return [torch.cat(list(comp)) for comp in ct.data]


def test_the_list_of_entries_is_the_backends():
    """NATIVE_ENTRIES is every HipBackend method with an `out` or `outs` parameter that stands for a whole op: the 21 from
    switch_key_native / cc_mult_evk to lt_matmul_bsgs_native (the step methods are out of scope; the sharded halves are
    HALF_ENTRIES, below)."""
    import inspect
    src = inspect.getsource(__import__("liberate_fhe_amd.fhe.backend", fromlist=["x"]))
    import re
    found = [m.group(1) for m in re.finditer(r"^    def (\w+)\(self, ([^)]*)\)", src, re.M)
             if re.search(r"\bouts?\b", m.group(2)) and (m.group(1).endswith("_native") or m.group(1) == "cc_mult_evk")]
    assert sorted(found) == sorted(NATIVE_ENTRIES) and len(NATIVE_ENTRIES) == 21


@pytest.mark.parametrize("fill", sorted(FENCE_FILLS))
def test_fenced_and_plain_runs_of_two_ops_give_equal_words(fill):
    plain, fenced = engine(), engine()
    fence = Fence(fenced, FENCE_FILLS[fill])
    res = []
    for eng in (plain, fenced):
        evk, rotk = synth.key_switch_key(eng, 3), synth.key_switch_key(eng, 4, origin="rotation key:1")
        a, b = synth.ciphertext(eng, 1, 0), synth.ciphertext(eng, 2, 0)
        keep = Untouched(a=a, b=b, evk=evk, rotk=rotk)
        res.append(words(eng.cc_mult(a, b, evk)) + words(eng.rotate_single(a, rotk)))
        keep.check(fill)
    assert len(fence.scratch) >= 3                      # the key switch's state, digits and sums at the least
    fence.check()
    assert all(torch.equal(x, y) for x, y in zip(*res))
    fence.refill()
    fence.check()


def scribble(t, offset, value=5):
    """one word `offset` words from the first word of t's view, whatever lies there"""
    t.as_strided((1,), (1,), t.storage_offset() + offset).fill_(value)


def stub_cc_dot(fault):
    """backend.cc_dot_native's signature; writes every output word, then commits `fault`"""
    def cc_dot_native(plan, ins, row0s, key, first_part, row_off, out, ws):
        if fault != "unwritten":
            out.fill_(7)
        ws.fill_(9)
        if fault == "before out":
            scribble(out, -1)
        elif fault == "behind out":
            scribble(out, out.numel() + 3)
        elif fault == "behind ws":
            scribble(ws, ws.numel())
        elif fault == "plan guard":
            scribble(plan, -7)
        elif fault == "operand":
            ins[0][0, 0] += 1
    return cc_dot_native


def run_stub(fault, fill=-1):
    eng = engine({"cc_dot_native": stub_cc_dot(fault)})
    fence = Fence(eng, fill)
    N = eng.ctx.N
    state = eng._ws("ks_state", (3, N), 0)              # stands for the plan: one of its scratch tensors
    ws = eng._ws("dot_ws", (3 * 3 * N,), 0)
    ins = [torch.arange(2 * N, dtype=torch.int64).view(2, N)]
    out = torch.empty((2, 3, N), dtype=torch.int64)
    keep = Untouched(ins=ins)
    return eng, fence, keep, lambda: eng.backend.cc_dot_native(state, ins, None, None, 0, 0, out, ws), out


def test_a_clean_stub_passes_and_its_output_arrives():
    eng, fence, keep, call, out = run_stub(None)
    call()
    keep.check()
    assert fence.calls == ["cc_dot_native"] and bool((out == 7).all()) and not fence.unwritten()
    assert all(f.buf.numel() == f.flat.numel() + 2 * fence.guard for f in fence.scratch.values())
    assert fence.guard == eng._rows(0, 0, True) * eng.ctx.N and fence.guard % 2 == 0


@pytest.mark.parametrize("fault,key,side,offset", [
    ("before out", "('cc_dot_native', 'out')", "before", 1),
    ("behind out", "('cc_dot_native', 'out')", "behind", 3),
    ("behind ws", "('dot_ws', ", "behind", 0),
    ("plan guard", "('ks_state', ", "before", 7)])
def test_a_word_outside_a_buffer_is_reported_where_it_fell(fault, key, side, offset):
    _, fence, _, call, _ = run_stub(fault)
    with pytest.raises(FenceError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith(key) and f"guard {side} the buffer" in msg and f"at offset {offset} (1 of" in msg, msg


def test_a_written_constant_equal_to_the_fill_is_still_seen_in_a_guard():
    """the guards hold a position-dependent pattern, not the fill: a kernel that writes the fill's own value outside is caught"""
    eng, fence, _, _, _ = run_stub(None)
    scribble(next(iter(fence.scratch.values())).body, -1, value=-1)
    with pytest.raises(FenceError):
        fence.check()


def test_a_modified_operand_is_reported():
    _, fence, keep, call, _ = run_stub("operand")
    call()
    with pytest.raises(AssertionError, match="operand 'ins' was modified.*1 words, first at \\(0, 0\\)"):
        keep.check("stub")


def test_an_output_never_written_does_not_pass_as_a_result():
    """it holds the fill: unwritten() names it, and its words differ from fill to fill (what the GPU file compares)"""
    got = []
    for fill in (FENCE_FILLS["ones"], FENCE_FILLS["max"]):
        _, fence, _, call, out = run_stub("unwritten", fill)
        call()
        assert fence.unwritten() == [("cc_dot_native", "out")]
        got.append(out.clone())
    assert not torch.equal(got[0], got[1])


def test_refill_skips_what_holds_constants():
    eng = engine(moddown_consts=lambda ws, *a: ws[:4].fill_(11),
                 make_plan=lambda ints, tensors, *a: tensors["md_ws"][:4].fill_(12))
    fence = Fence(eng, FENCE_FILLS["max"])
    a, b, c = (eng._ws(k, (64,), 0) for k in ("md_a", "md_b", "plain"))
    eng.backend.moddown_consts(a, 2, 3, 2, eng.ctx.N, None, None)
    eng.backend.make_plan({}, {"md_ws": b, "state": c}, None, None, None, None)
    c.fill_(0)
    fence.refill()
    assert a[:4].tolist() == [11] * 4 and b[:4].tolist() == [12] * 4 and bool((c == FENCE_FILLS["max"]).all())
    fence.check()


def test_the_halves_of_a_sharded_op_are_the_backends_and_are_fenced():
    """HALF_ENTRIES is every method of the backend's section "the halves of an op around the digit exchange" that launches; the
    fence wraps each one a backend has.  A stub plan_fwd (no `out`: the guard check of all scratch on the way out) that writes
    one word behind the exchange buffer ks_digits_all is reported at that buffer; a stub cc_mult_post handed out = None
    (which = 1: plan scratch only) runs, and with an `out` it gets a fenced one whose words arrive."""
    import inspect
    from liberate_fhe_amd.fhe import backend as B
    src = inspect.getsource(B.HipBackend)
    section = src[src.index("the halves of an op around the digit exchange"):src.index("def cc_mult_evk(")]
    import re
    assert sorted(re.findall(r"^    def (\w+)\(self", section, re.M)) == sorted(HALF_ENTRIES)

    def plan_fwd(plan, digits, first, count, relin):
        scribble(digits, digits.numel())

    def cc_mult_post(plan, key, first_part, row_off, out, which=3):
        if out is not None:
            out.fill_(7)

    eng = engine({"plan_fwd": plan_fwd, "cc_mult_post": cc_mult_post})
    fence = Fence(eng, -1)
    N = eng.ctx.N
    buf = eng._ws("ks_digits_all", (3, N), 0)
    eng.backend.cc_mult_post(None, None, 0, 0, None, which=1)
    out = torch.empty((2, 3, N), dtype=torch.int64)
    eng.backend.cc_mult_post(None, None, 0, 0, out)
    assert fence.calls == ["cc_mult_post", "cc_mult_post"] and bool((out == 7).all()) and not fence.unwritten()
    with pytest.raises(FenceError) as e:
        eng.backend.plan_fwd(None, buf, 0, 1, True)
    msg = str(e.value)
    assert msg.startswith("('ks_digits_all', ") and "guard behind the buffer" in msg and "at offset 0 (1 of" in msg, msg
