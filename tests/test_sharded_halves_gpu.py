"""The native halves of a limb-sharded op — lf_cc_mult_evk_pre / _post, lf_switch_key_pre / _post, lf_ks_plan_fwd — as STEPS, in one
process, no process group and no graphs: H = ckks_engine(devices=["cuda:0"] * W) hands out rank d's plan for every logical
device d (H._op_plan(level, d): `dig_nparts` of `nparts` digits, `own`, `row_off`, `first_part` of ITS rows), the test drives
the halves of every device through H.backend and does the digit exchange by hand: each owner's state[src_row : src_row + nrows]
into rows row0 .. of a storage-order buffer per device (the positions of _ks_tables(level)["groups"], as _exchange_digits takes
them), the rest of the buffer at -1.

Ground truth: the checker engine on W CPU devices (tests/oracle_backend.OracleBackend), shard d of its result and its digit
state of device d.  Bit-exact; sets, worlds and levels are those of tests/test_sharded_edges_gpu.py (WORLDS).

  the wire        after switch_key_pre, after cc_mult_pre(which=3) and after which=1 followed by which=2, plan.state of device d
                  equals the checker's ks_digits words of device d: these are the words a peer reads off the wire, and a wrong
                  one fails HERE, not at the result.
  plan_fwd        in four orders, for relin 0 (the switch kind) and 1 (cc_mult): own runs first and then the foreign runs (the
                  engine's order), one call over 0 .. nparts, digit by digit descending, foreign runs first.  Each starts from
                  plan.ext and plan.sum filled with -1, so nothing an earlier order left can stand in for a digit it did not
                  write; each is followed by a post half and compared with the checker, so all four are identical.
  post            which=3 and which=1 followed by which=2, on the raw key pack and on the planes pack (of a compact_key key for
                  the "top" keys), one combination per order; `out` is -1-filled with a guard row behind it (guard_ok / body).
                  cc_mult; rotate_single by 1 and by -(N/2 - 1); conjugate; a plain switch_key (pinv 0).
  patterns        every pair of PAIRS of tests/test_engine_edges_gpu.py at every tested level (one test per level); cc_mult on
                  pre_rescale_ciphertext operands: 0, round_at - 1, round_at, round_at + 1, q_drop - 1 in the dropped row, which
                  reaches every device as a copy of its OWNER's row.  Every world has a product whose dropped row belongs to another
                  device than 0 (owners_not_zero(), asserted): among its tested levels, or — sb40_K1 over 2 ranks, whose levels
                  1 and 7 are fed by rank 0's rows — the product into level 2, added for that.
  refusals        sixteen: which = 0 and 4 of cc_mult_pre, cc_mult_post and switch_key_post (switch_key_pre takes no `which`); for
                  relin 0 and 1, plan_fwd with first + count > nparts (twice: a count and a first past the end), count < 0,
                  first < 0 and a null `digits`.  LF_ERR_ARG before any launch: state, ext, sum, digits and out at their fill."""
import ctypes
import warnings

import pytest
import torch

from tests.helpers import StepTables, body, edge_ciphertext, edge_key, pre_rescale_ciphertext
from tests.test_engine_edges_gpu import PAIRS, engines, same
from tests.test_sharded_edges_gpu import WORLDS, rule_levels

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", category=UserWarning)


def runs(groups, d):
    """(own runs [(first digit, digits)], maximal foreign runs) of device d: what _sharded_schedule hands the engine"""
    own, foreign, run = [], [], None
    for owner, first, count, _, _, _ in list(groups) + [(d, None, 0, 0, 0, 0)]:
        if owner == d:
            if run is not None:
                foreign.append(run)
                run = None
            if first is not None:
                own.append((first, count))
        else:
            run = (first, count) if run is None else (run[0], run[1] + count)
    return own, foreign


def orders(groups, d, nparts):
    own, foreign = runs(groups, d)
    return (("engine", own + foreign), ("one call", [(0, nparts)]), ("descending", [(p, 1) for p in reversed(range(nparts))]),
            ("foreign first", foreign + own))


def exchange(H, level, alive, states):
    """the digit exchange by hand: {device: [total_rows, N] buffer}, every row some owner's, copied from ITS state"""
    tabs = H._ks_tables(level)
    N = H.ctx.N
    bufs = {}
    for t in alive:
        buf = torch.full((tabs["total_rows"], N), -1, dtype=torch.int64, device="cuda:0")
        for owner, first, count, row0, nrows, src_row in tabs["groups"]:
            buf[row0:row0 + nrows].copy_(states[owner][src_row:src_row + nrows])
        bufs[t] = buf
    return bufs


def packs_of(H, key, compact):
    """[(name, per-device packs)]: the raw pack the key's tensors are views of, the planes copy the fused path reads"""
    raw = [p.clone() for p in H._key_packs[id(H._key_anchor(key))]["packs"]]
    planes = H._key_pack(key)
    if compact:
        assert H.compact_key(key) > 0
        assert H._key_pack(key) is planes
    return [("raw", raw), ("planes of a compact key" if compact else "planes", planes)]


def checker_state(C, level, d):
    return C._ws("ks_state", (C._rows(d, level, False), C.ctx.N), d)


def _halves_case(H, C, level, pattern, kpat, seed, compact, switch=True):
    """every op of one (level, pattern pair) through the halves of every device alive at the level (switch=False: cc_mult only)"""
    from liberate_fhe_amd.fhe import encdec
    from liberate_fhe_amd.fhe.backend import _ds
    be = H.backend
    N = H.ctx.N
    alive = list(range(H.len_devices[level]))
    tabs = H._ks_tables(level)
    nparts = len(tabs["order"])
    plans = {d: H._op_plan(level, d) for d in alive}
    states = {d: H._ws("ks_state", (plans[d][0].ell, N), d) for d in alive}
    T = {d: StepTables(H, level, d) for d in alive}
    tag0 = f"level {level} {pattern}/{kpat}"

    def finish(kind, want, keypacks, post, what):
        """exchange, then per device the four orders of plan_fwd, each with its own post form and key format"""
        bufs = exchange(H, level, alive, states)
        forms = ((3, 0), (12, 1), (3, 1), (12, 0))
        for d in alive:
            plan = plans[d][0]
            scratch = (H._ws("ks_ext", (nparts, plan.ell + plan.K, N), d), H._ws("ks_sum", (2, plan.ell + plan.K, N), d))
            assert scratch[0].data_ptr() == plan.ext and scratch[1].data_ptr() == plan.sum
            for (oname, order), (which, fmt) in zip(orders(tabs["groups"], d, nparts), forms):
                for t in scratch:       # every order starts from hostile scratch: what an earlier order left cannot stand in
                    t.fill_(-1)         # for a digit this one did not write, or for a post half that did nothing
                for first, count in order:
                    be.plan_fwd(plans[d][0], bufs[d], first, count, kind == "mult")
                kname, kp = keypacks[fmt]
                out = T[d].new(2, plans[d][0].ell, N)
                if which == 3:
                    post(d, kp[d], body(out), 3)
                else:
                    post(d, kp[d], None, 1)
                    post(d, kp[d], body(out), 2)
                w = torch.stack([want.data[0][d], want.data[1][d]])
                same(out, w, f"{what}: device {d}, plan_fwd order '{oname}', post which={which}, {kname} key, {tag0}")

    # ---- the switch kind: rotations by 1 and by -(N/2 - 1), conjugate, plain switch_key ----
    delta2 = -(N // 2 - 1)
    ops = (("rotate 1", encdec.galois_exponent(N, 1), True, f"rotation key:1", C.rotate_single),
           (f"rotate {delta2}", encdec.galois_exponent(N, delta2), True, f"rotation key:{delta2}", C.rotate_single),
           ("conjugate", encdec.conjugation_exponent(N), False, "conjugation key", C.conjugate),
           ("switch_key", None, False, "key switch key", C.switch_key))
    for i, (name, exponent, canonical, origin, c_op) in enumerate(ops if switch else ()):
        ct_h, ct_c = (edge_ciphertext(e, level, pattern, seed + i) for e in (H, C))
        key_h, key_c = (edge_key(e, kpat, seed + 10 + i, origin=origin) for e in (H, C))
        want = c_op(ct_c, key_c)
        pinv = 0 if exponent is None else pow(exponent, -1, 2 * N)
        for d in alive:
            states[d].fill_(-1)
            be.switch_key_pre(plans[d][0], ct_h.data[1][d], pinv, canonical)
            assert torch.equal(states[d].cpu(), checker_state(C, level, d)), f"{name}: the digits device {d} sends, {tag0}"
        keypacks = packs_of(H, key_h, compact and kpat == "top")

        def post(d, kp, out, which):
            plan, _, first_part, row_off = plans[d]
            be.switch_key_post(plan, ct_h.data[0][d], pinv, canonical, kp, first_part, row_off, out, which=which)
        finish("switch", want, keypacks, post, name)

    # ---- cc_mult into the level: operands one level up, the dropped row a copy of its owner's ----
    if level == 0:
        return
    a_h, b_h = pre_rescale_ciphertext(H, level - 1, pattern, seed + 20), pre_rescale_ciphertext(H, level - 1, pattern, seed + 21, shift=1)
    a_c, b_c = pre_rescale_ciphertext(C, level - 1, pattern, seed + 20), pre_rescale_ciphertext(C, level - 1, pattern, seed + 21, shift=1)
    evk_h, evk_c = edge_key(H, kpat, seed + 30), edge_key(C, kpat, seed + 30)
    want = C.cc_mult(a_c, b_c, evk_c)
    owner = H.ntt.p.rescaler_loc[level - 1]
    polys = {d: [t.contiguous() for t in (a_h.data[0][d], a_h.data[1][d], b_h.data[0][d], b_h.data[1][d])]
             for d in range(H.len_devices[level - 1])}
    for form in ((3,), (1, 2)):
        for d in alive:
            rbuf = torch.stack([t[0] for t in polys[owner]]).contiguous()            # what the owner's message leaves on device d
            skip = N * 8 if owner == d else 0
            ins = (ctypes.c_void_p * 4)(*[t.data_ptr() + skip for t in polys[d]])
            row0s = (ctypes.c_void_p * 4)(*[rbuf[k].data_ptr() for k in range(4)])
            states[d].fill_(-1)
            for which in form:
                be.cc_mult_pre(plans[d][0], ins if which & 1 else None, row0s if which & 1 else None, _ds(rbuf)[1], which=which)
            assert torch.equal(states[d].cpu(), checker_state(C, level, d)), \
                f"cc_mult pre which={form}: the digits device {d} sends, {tag0} (the dropped row's owner: {owner})"
    keypacks = packs_of(H, evk_h, compact and kpat == "top")

    def post(d, kp, out, which):
        plan, _, first_part, row_off = plans[d]
        be.cc_mult_post(plan, kp, first_part, row_off, out, which=which)
    # (the operand stack x4 of every device is the one its LAST pre left: which = 1 then 2; post reads it for the fold)
    finish("mult", want, keypacks, post, "cc_mult")


def owners_not_zero(C, levels):
    return [lv for lv in levels if lv >= 1 and C.ntt.p.rescaler_loc[lv - 1] != 0]


def step_levels():
    """[(world, level, cc_mult only)]: every tested level of every world, and the product into the first level that is not tested
    anyway — level 0 has no product INTO it — and, where no tested level's dropped row belongs to another device than 0 (sb40_K1
    over 2 ranks: its levels 1 and 7 are fed by rank 0's rows), into the next one as well (level 2, dropped by rank 1)."""
    out = []
    for world, levels in WORLDS.items():
        out += [(world, lv, False) for lv in levels]
        out += [(world, lv, True) for lv in [lv for lv in (1, 2) if lv not in levels][:2 if world == ("sb40_K1", 2) else 1]]
    return out


STEP_LEVELS = step_levels()


@pytest.mark.parametrize("world,level,mult_only", STEP_LEVELS,
                         ids=[f"{n}-W{w}-{'into' if m else 'L'}{lv}" for (n, w), lv, m in STEP_LEVELS])
def test_the_halves_of_every_device_equal_the_checker_step_by_step(world, level, mult_only):
    """every pair of PAIRS at every tested level (one test per level: the levels are in the ids)"""
    name, W = world
    H, C = engines(name, W)
    levels = WORLDS[world]
    assert rule_levels(C, W, False) == levels
    products = list(levels) + [lv for w, lv, m in STEP_LEVELS if w == world and m]
    assert owners_not_zero(C, products), "no product whose dropped row belongs to another device than 0"
    for pi, (pattern, kpat) in enumerate(PAIRS):
        _halves_case(H, C, level, pattern, kpat, 400 + 50 * level + 7 * pi + (500 if mult_only else 0), compact=pi == 0,
                     switch=not mult_only)


def test_the_halves_refuse_bad_arguments_before_any_launch():
    """Sixteen refusals — which = 0 and 4 of the three halves that take it; five bad (digits, first, count) of plan_fwd for relin 0
    and 1 — return LF_ERR_ARG with nothing launched: the plan's state, ext and sum, the digit buffer and the output hold their fill."""
    from liberate_fhe_amd._native import LF_ERR_ARG, lib
    from liberate_fhe_amd.fhe.backend import _ds
    H, C = engines("sb41_K2", 2)
    level, d, N = 1, 0, H.ctx.N
    plan, _, first_part, row_off = H._op_plan(level, d)
    key = edge_key(H, "random", 77)
    kp = H._key_pack(key)[d]
    base, ps, cs = H.backend._key_args(kp, first_part)
    fmt = H.backend._kfmt(kp)
    tabs = H._ks_tables(level)
    state = H._ws("ks_state", (plan.ell, N), d)
    ext = H._ws("ks_ext", (plan.nparts, plan.ell + plan.K, N), d)
    summ = H._ws("ks_sum", (2, plan.ell + plan.K, N), d)
    digits = torch.full((tabs["total_rows"], N), -1, dtype=torch.int64, device="cuda:0")
    out = torch.full((2, plan.ell, N), -1, dtype=torch.int64, device="cuda:0")
    c = torch.full((plan.ell, N), 1, dtype=torch.int64, device="cuda:0")
    for t in (state, ext, summ):
        t.fill_(-1)
    st = _ds(out)[1]
    ptrs = (ctypes.c_void_p * 4)(*[c.data_ptr()] * 4)
    p, o0, o1 = ctypes.byref(plan), out.data_ptr(), out.data_ptr() + out.stride(0) * 8
    codes = {}
    for which in (0, 4):
        codes["cc_mult_pre", which] = lib.lf_cc_mult_evk_pre(p, ptrs, ptrs, which, st)
        codes["cc_mult_post", which] = lib.lf_cc_mult_evk_post(p, base, ps, cs, row_off, fmt, o0, o1, which, st)
        codes["switch_key_post", which] = lib.lf_switch_key_post(p, c.data_ptr(), 1, 1, base, ps, cs, row_off, fmt, o0, o1, which, st)
    n = plan.nparts
    for relin in (0, 1):
        for what, (dg, first, count) in {"past the end": (digits.data_ptr(), 1, n), "first past the end": (digits.data_ptr(), n + 1, 0),
                                         "negative count": (digits.data_ptr(), 0, -1), "negative first": (digits.data_ptr(), -1, 1),
                                         "null digits": (None, 0, 1)}.items():
            codes["plan_fwd", what, relin] = lib.lf_ks_plan_fwd(p, dg, first, count, relin, st)
    torch.cuda.synchronize()
    assert len(codes) == 16 and all(v == LF_ERR_ARG for v in codes.values()), codes
    for t, what in ((state, "state"), (ext, "ext"), (summ, "sum"), (digits, "digits"), (out, "out")):
        assert bool((t == -1).all()), f"a refused half wrote {what}"
    assert bool((c == 1).all())
