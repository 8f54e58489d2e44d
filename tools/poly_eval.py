"""weighted_sums and poly_eval against the ways to write them without the new layer, in one process on one GPU:
    python tools/poly_eval.py [--presets silver,gold] [--ks 3,7,15] [--gs 1,4] [--degrees 7,15,31,63] [--min-seconds 0.3] [--rounds 3]
(a) for every (preset, k, G) at level 0, G weighted sums of k ciphertexts with consts:
    native   weighted_sums(cts, w, consts)                         one native call (lf_weighted_sums), its device table of the
                                                                   weights kept from the warm-up (the engine keeps it per weights)
    cold     the same with that table dropped before every call    (new weights every time: G k (l + 1) host reductions + an upload)
    chain    the ops that define it, written out: _scale_rows per term, the cc_add chain, rescale, add_scalar
(b) for every (preset, degree) at level 0, a power-basis polynomial with random coefficients:
    poly     poly_eval(ct, coeffs, evk)                            Paterson-Stockmeyer
    terms    add_scalar(mult_scalar(x, c_1), c_0), then auto_cc_add of mult_scalar(pow(x, i), c_i) for every i >= 2
The forms of a point are timed alternately with device events after a warm-up of each, every timing over at least --min-seconds
of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its rounds) is
reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads and the ratios.
    python tools/poly_eval.py --trace gold:sums:15:4 [--calls 10] [--form native|cold|chain]
    python tools/poly_eval.py --trace gold:poly:31 [--calls 10] [--form poly|terms]
runs only that form at that point (for a kernel trace taken from outside, the program in a process of its own).
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


def measure(forms, rounds, min_seconds):
    for fn in forms.values():
        fn()
    times = {f: [] for f in forms}
    for _ in range(rounds):
        for f, fn in forms.items():
            times[f].append(timed(fn, min_seconds))
    med = {f: statistics.median(t) for f, t in times.items()}
    spread = {f: (max(t) - min(t)) / med[f] for f, t in times.items()}
    return med, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--ks", default="3,7,15")
    ap.add_argument("--gs", default="1,4")
    ap.add_argument("--degrees", default="7,15,31,63")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", default=None, help="preset:sums:k:G or preset:poly:degree — run one form alone, --calls times")
    ap.add_argument("--form", default=None, choices=("native", "cold", "chain", "poly", "terms"))
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("poly_eval: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    names = args.presets.split(",")
    sums = [(int(k), int(G)) for k in args.ks.split(",") if k for G in args.gs.split(",") if G]
    degrees = [int(d) for d in args.degrees.split(",") if d]
    if args.trace:
        f = args.trace.split(":")
        names = [f[0]]
        sums = [(int(f[2]), int(f[3]))] if f[1] == "sums" else []
        degrees = [int(f[2])] if f[1] == "poly" else []
    result = {"unit": "us per call, level 0", "sums": [], "poly": []}
    rng = np.random.default_rng(1)
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        assert eng._native_level(0) is not None and eng._native_level(1) is not None
        evk = synth.key_switch_key(eng, 77)
        pool = [synth.ciphertext(eng, 50 + i, 0) for i in range(4)]
        for k, G in sums:
            cts = [pool[i % 4] for i in range(k)]
            w, consts = rng.uniform(-1, 1, (G, k)), rng.uniform(-1, 1, G)

            def chain():
                outs = []
                for row, c in zip(w, consts):
                    acc = None
                    for ct, x in zip(cts, row):
                        s = int(x * eng.scale * np.sqrt(eng.deviations[1]) + 0.5)
                        term = eng._scale_rows(ct, eng._row_scalars(s, 0, True))
                        acc = term if acc is None else eng.cc_add(acc, term)
                    outs.append(eng.add_scalar(eng.rescale(acc), c))
                return outs

            def cold():
                getattr(eng, "_wsum_tables", {}).clear()
                return eng.weighted_sums(cts, w, consts)

            forms = {"native": lambda: eng.weighted_sums(cts, w, consts), "cold": cold, "chain": chain}
            if args.trace:
                for _ in range(args.calls):
                    forms[args.form or "native"]()
                torch.cuda.synchronize()
                continue
            med, spread = measure(forms, args.rounds, args.min_seconds)
            point = {"preset": name, "k": k, "G": G, **{f: round(med[f], 1) for f in forms},
                     **{f"spread_{f}": round(spread[f], 4) for f in forms},
                     "chain_over_native": round(med["chain"] / med["native"], 2), "chain_over_cold": round(med["chain"] / med["cold"], 2)}
            result["sums"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        x = pool[0]
        for d in degrees:
            coeffs = rng.uniform(-1, 1, d + 1)

            def terms():
                acc = eng.add_scalar(eng.mult_scalar(x, coeffs[1]), coeffs[0])
                for i in range(2, d + 1):
                    acc = eng.auto_cc_add(acc, eng.mult_scalar(eng.pow(x, i, evk), coeffs[i]))
                return acc

            forms = {"poly": lambda: eng.poly_eval(x, coeffs, evk), "terms": terms}
            if args.trace:
                for _ in range(args.calls):
                    forms[args.form or "poly"]()
                torch.cuda.synchronize()
                continue
            med, spread = measure(forms, args.rounds, args.min_seconds)
            point = {"preset": name, "degree": d, "depth": eng.poly_depth(d), **{f: round(med[f], 1) for f in forms},
                     **{f"spread_{f}": round(spread[f], 4) for f in forms}, "terms_over_poly": round(med["terms"] / med["poly"], 2)}
            result["poly"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        del eng, evk, pool, x
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
