"""Record tests/golden/reference_results.json, and the ciphertext files tests/golden/reference_saved_c1_x<devices>.pkl, by
running the bodies of the reference comparisons on the REFERENCE (its Python layers imported from its source tree, its CUDA
modules replaced by the C oracle: see refdriver.py):

  tests/test_engine_vs_reference.py      precomputed tables, hot path on real keys
  tests/test_evaluator_vs_reference.py   scalar / plaintext operands, statistics, host form and save / load, multiparty
  tests/test_generate_engine_cpu.py      prime chains, the shipped scale-prime table
  tests/test_w30_cpu.py                  the 30-bit context
  tests/test_csprng_cpu.py               the Csprng class over the checker's kernels

    python tests/golden/make_golden_reference.py      # where the reference's source tree is (refdriver.REFERENCE_SRC)

The tests then run the same bodies on this repo's engine and compare with what is recorded here: fingerprints
(tests/helpers.fingerprint), no reference source text.
"""
import os
import pickle
import sys
import tempfile
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

from tests import csprng_streams as cs  # noqa: E402
from tests import test_csprng_cpu as TC  # noqa: E402
from tests import test_engine_vs_reference as TE  # noqa: E402
from tests import test_evaluator_vs_reference as TV  # noqa: E402
from tests import test_generate_engine_cpu as TG  # noqa: E402
from tests import test_w30_cpu as TW  # noqa: E402
from tests.golden import refdriver as rd  # noqa: E402
from tests.helpers import Recorded, fingerprint  # noqa: E402


class _Dev:
    type = "cuda"


class _CudaLike(torch.Tensor):
    @property
    def device(self):
        return _Dev()


def ref_host(ref, text):
    """ref.move_to(text, "gpu2cpu"): the reference insists on CUDA tensors before downloading; on the CPU stand-in
    relax that one check."""
    orig = ref.download_to_cpu

    def download(gpu_data, level, include_special):
        fake = [t.clone() for t in gpu_data]
        for t in fake:
            t.__class__ = _CudaLike
        return orig(fake, level, include_special)
    ref.download_to_cpu = download
    try:
        return ref.move_to(text, "gpu2cpu")
    finally:
        ref.download_to_cpu = orig


def world(ref):
    w = TV.make_world(ref)
    w["record"] = True
    return w


def move_save_load(n_dev):
    """Host forms, c1 through the reference's save(), and this repo's saved evk through the reference's load()."""
    w = world(rd.reference_engine(n_dev, **TE.SMALL))
    ref, rec = w["e"], TV.recorded(w, "move_save_load")
    for name in ("c1", "evk", "gk"):
        rec.check("host " + name, TV.host_rows(ref_host(ref, w[name]), len(ref.ctx.q)))
    with open(TV.saved_c1_path(n_dev), "wb") as f:          # the reference's save(): a pickle of the host form
        pickle.dump(ref_host(ref, w["c1"]), f)
    me = TV.make_world(TE.mine(n_dev, **TE.SMALL))
    assert fingerprint(me["evk"]) == fingerprint(w["evk"])
    path = os.path.join(tempfile.mkdtemp(prefix="lfa_golden_"), "mine.pkl")
    me["e"].save(me["evk"], path)
    assert fingerprint(ref.load(path, move_to_gpu=True)) == fingerprint(w["evk"])
    rec.check("saved evk file", TV.saved_file(path))


def main():
    if not rd.reference_available():
        raise SystemExit(f"the reference's source tree is not at {rd.REFERENCE_SRC}")
    for n in (1, 2, 3):
        TE.check_tables(rd.reference_engine(n, **TE.SMALL), Recorded(f"precomputed_tables[{n}]", record=True))
    for n in (1, 2):
        TE.hot_path(rd.reference_engine(n, **TE.SMALL), Recorded(f"hot_path[{n}]", record=True))
    for n in (1, 2):
        w = world(rd.reference_engine(n, **TE.SMALL))
        for body in (TV.scalar_operands, TV.plaintext_operands, TV.multiparty_protocol):
            body(w, TV.recorded(w, body.__name__))
        move_save_load(n)
    w = world(rd.reference_engine(1, **TV.DEEP))
    TV.statistics_and_powers(w, TV.recorded(w, "statistics_and_powers"))

    for logN, scale_bits in sorted(TG.EXPECTED):
        Recorded(f"chain[{logN},{scale_bits}]", record=True).check(
            "q", TG.chain(lambda: rd.reference_context(**TG.ctx_params(logN, scale_bits))))
    rec = Recorded("scale_prime_pools", record=True)
    table = pickle.load(open(os.path.join(rd.REFERENCE_SRC, "liberate/fhe/cache/resources/scale_primes.pkl"), "rb"))
    for (sb, N), pool in table.items():
        rec.check(f"{sb},{N}", TG.scale_pool_digest(pool))

    TW.check_context30(rd.reference_context(**TW.CONTEXT30), Recorded("context30", record=True))

    cfg = cs.STREAM_CONFIGS["small"]
    TC.check_class_live(rd.reference_csprng(cfg["num_coefs"], cfg["num_channels"], cfg["num_repeating_channels"], cfg["n_dev"],
                                            cs.STREAM_KEY, cs.STREAM_NONCE), Recorded("csprng_class_live", record=True))
    Recorded.save()
    print("wrote", Recorded.PATH)


if __name__ == "__main__":
    main()
