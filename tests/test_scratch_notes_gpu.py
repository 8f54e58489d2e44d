"""The library's notes of the format it left in scratch that crosses native calls (csrc/ckks_hip.hip: lf_fmt_note / lf_fmt_expect)
against memory the caller's allocator recycles.  Nobody unregisters a freed buffer, so a note outlives its buffer; a flip of
LF_TUNE_WS_EXTRA_STAGE (the workspace split of lf_ntt_ws, another family of formats) must not turn such a note of a DIGIT format
into a refusal of digits a caller wrote there by hand, while a flip of LF_TUNE_DIGIT_PLANES between lf_ks_fwd and lf_ks_tail is
still refused.  Which test's tensors land on which freed block depends on the allocator and on when Python collects an engine:
here the block is shared on purpose."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digit_words(T, op, planes):
    """Extended digits written by hand in the format lf_ks_fwd leaves them in (tests/test_engine_edges_gpu.py): integer-class
    rows lazy words, fp64-class rows plain canonical residues, as raw words or as 32-bit low words + 16-bit high halves."""
    from tests.helpers import SMALL_PRIME_LIMIT
    q = np.array(T.q_all)
    small = q < SMALL_PRIME_LIMIT
    x = np.where(small[None, :, None], op["ext"] % q[None, :, None], op["ext"])
    words = x.copy()
    if planes:
        for r in np.nonzero(small)[0]:
            row = np.zeros((T.nparts, T.N), dtype=np.int64)
            row.view(np.uint32)[:, :T.N] = (x[:, r] & 0xffffffff).astype(np.uint32)
            row.view(np.uint16)[:, 2 * T.N:3 * T.N] = (x[:, r] >> 32).astype(np.uint16)
            words[:, r] = row
    return words


def stale_note_walk():
    """The body of the test below; it flips process-wide knobs, so it runs in a process of its own."""
    from liberate_fhe_amd._native import LF_ERR_STATE, HipError, lib
    from liberate_fhe_amd.fhe import ckks_engine
    from tests.helpers import SMALL_PRIME_LIMIT, StepTables, edge_param_sets, step_operands
    sets = edge_param_sets()
    A = ckks_engine(devices=["cuda:0"], **sets["sb45_K4"])
    B = ckks_engine(devices=["cuda:0"], **sets["sb20"])
    TA, TB = StepTables(A, 0), StepTables(B, 0)

    def planes_of(T):
        small = np.array(T.q_all) < SMALL_PRIME_LIMIT
        return lib.lf_tune(3, -1) == 1 and bool(small.any()) and not bool(small.all())

    assert not planes_of(TA) and planes_of(TB)      # A leaves raw words, B reads planes
    wa, wb = TA.nparts * TA.rows * TA.N, TB.nparts * TB.rows * TB.N
    arena = torch.zeros(max(wa, wb), dtype=torch.int64, device="cuda:0")
    tmp_a, tmp_b = arena[:wa].view(TA.nparts, TA.rows, TA.N), arena[:wb].view(TB.nparts, TB.rows, TB.N)
    op_a, op_b = step_operands(TA, "random", "random", 3), step_operands(TB, "random", "random", 7)
    key_b = TB.put(op_b["key"])
    words = digit_words(TB, op_b, True)

    def tail(tmp):
        got = torch.empty((2, TB.rows, TB.N), dtype=torch.int64, device="cuda:0")
        B.backend.ks_tail(TB.nparts, TB.rows, TB.logN, key_b, TB.first_part, TB.row_off, tmp, got, TB.ipsi, TB.ninv, TB.c_all)
        return got.cpu()

    want = tail(TB.put(words))                       # memory nobody noted
    # engine A's key switch leaves its digits, and a note "raw words", in the arena ...
    A.backend.ks_fwd(TA.put(op_a["state_hi"]), 0, TA.nparts, TA.rows, TA.logN, TA.e_desc, TA.E, TA.Ed, tmp_a, TA.psi, TA.c_all)
    torch.cuda.synchronize()
    # ... the workspace knob is flipped and restored (no digit format depends on it) ...
    old = lib.lf_tune(4, -1)
    lib.lf_tune(4, 1 - old), lib.lf_tune(4, old)
    # ... and the block, recycled, takes hand-written digits of engine B in planes: read on trust
    tmp_b.copy_(torch.from_numpy(words))
    assert torch.equal(tail(tmp_b), want)
    # the hazard the notes exist for is still refused: lf_ks_fwd under planes, LF_TUNE_DIGIT_PLANES flipped, lf_ks_tail
    B.backend.ks_fwd(TB.put(op_b["state_hi"]), 0, TB.nparts, TB.rows, TB.logN, TB.e_desc, TB.E, TB.Ed, tmp_b, TB.psi, TB.c_all)
    torch.cuda.synchronize()
    lib.lf_tune(3, 0)
    try:
        with pytest.raises(HipError, match=str(LF_ERR_STATE)):
            tail(tmp_b)
    finally:
        lib.lf_tune(3, 1)


@pytest.mark.gpu
def test_a_workspace_knob_flip_does_not_age_stale_digit_notes():
    """In a fresh child process (tests/test_cc_dot_gpu.py says why knob flips stay out of the suite's process)."""
    import subprocess
    import sys
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_scratch_notes_gpu import stale_note_walk; stale_note_walk()"
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
