"""linear_transform against the loop of existing ops it replaces (one ciphertext, k rotated diagonals + the step-0 one), in one process:
    python tools/linear_transform.py [--presets silver,gold] [--ks 1,2,4,8,16] [--min-seconds 0.5]
The loop is   acc = mc_mult(d0, ct); for r, dg in zip(rotate_hoisted(ct, keys), diags): acc = cc_add(acc, mc_mult(dg, r))
(plaintext encode, four transforms and a rescale per diagonal); linear_transform runs on pre-encoded diagonals.  For every
(preset, k) the two forms are timed alternately with device events after a warm-up, each over at least --min-seconds of work,
three rounds, the median kept.  Prints one JSON line: microseconds per call for each form and their ratio (loop / linear_transform).
    python tools/linear_transform.py --trace gold:8 [--calls 20]
runs only linear_transform at that point (for a kernel trace taken from outside, the program in a process of its own).
Synthetic keys and ciphertexts (utils/synth.py): the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")

from tools.hoisted_rotations import timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", default=None, help="preset:k — run linear_transform alone, --calls times")
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("linear_transform: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    names, ks = args.presets.split(","), [int(k) for k in args.ks.split(",")]
    if args.trace:
        names, ks = [args.trace.split(":")[0]], [int(args.trace.split(":")[1])]
    result = {"unit": "us per call (k rotated diagonals + step 0)", "points": []}
    rng = np.random.default_rng(1)
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        keys = [synth.key_switch_key(eng, 100 + i, origin=f"rotation key:{i + 1}") for i in range(max(ks))]
        ct = synth.ciphertext(eng, 7, 0)
        vecs = {s: rng.uniform(-1, 1, eng.num_slots) + 1j * rng.uniform(-1, 1, eng.num_slots) for s in range(max(ks) + 1)}
        for k in ks:
            enc = eng.encode_diagonals({s: vecs[s] for s in range(k + 1)}, 0)

            def loop():
                acc = eng.mc_mult(vecs[0], ct)
                for s, r in enumerate(eng.rotate_hoisted(ct, keys[:k])):
                    acc = eng.cc_add(acc, eng.mc_mult(vecs[s + 1], r))
                return acc

            lt = lambda: eng.linear_transform(ct, enc, keys[:k])
            if args.trace:
                for _ in range(args.calls):
                    lt()
                torch.cuda.synchronize()
                continue
            loop(), lt()
            t_loop, t_lt = [], []
            for _ in range(args.rounds):
                t_loop.append(timed(loop, args.min_seconds))
                t_lt.append(timed(lt, args.min_seconds))
            a, b = statistics.median(t_loop), statistics.median(t_lt)
            result["points"].append({"preset": name, "k": k, "loop_of_existing_ops": round(a, 1), "linear_transform": round(b, 1),
                                     "ratio": round(a / b, 3)})
            print(json.dumps(result["points"][-1]), file=sys.stderr, flush=True)
            del enc
        del eng, keys, ct
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
