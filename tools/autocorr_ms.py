#!/usr/bin/env python3
"""Device time of the sequence autocorrelation next to the pick call, on one record.

The benchmark's workload (synthetic(length), MFE, annealing 5 -> 0 over 300 steps)
is recorded for --steps steps in chunks of 300; then Engine.picks and
Engine.autocorr run --repeat times each on that record and the HIP-event times
(adx_last_pick_ms, adx_last_autocorr_ms) are printed as one JSON line per call,
then a summary line.

    python tools/autocorr_ms.py [--walkers 4096] [--length 100] [--steps 3000]
                                [--max-lag 500] [--discard 100] [--window 500] [--repeat 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--max-lag", type=int, default=500)
    ap.add_argument("--discard", type=int, default=100)
    ap.add_argument("--window", type=int, default=500)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fold", choices=("mfe", "pf"), default="mfe")
    a = ap.parse_args()
    from addapt_amd import native, workloads

    tmpl, active = workloads.synthetic(a.length)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=300)
    eng = native.Engine(tmpl, [active], workloads.config_objective(a.length, bppm=False), aptamer=apt, thermostat=th,
                        fold_mode=a.fold)
    gids = list(range(a.walkers))
    eng.walkers_init(gids, workloads.walker_sequences(tmpl, [active], a.walkers, seed_base=1000))
    eng.record(a.steps)
    run_ms, left = 0.0, a.steps
    while left > 0:
        n = min(300, left)
        eng.run_steps(n)
        run_ms += eng.last_kernel_ms()
        left -= n
    rows = []
    for k in range(a.repeat):
        picks, _ = eng.picks(a.window)
        pick_ms, replay_ms = eng.last_pick_ms()
        ac = eng.autocorr(a.max_lag, a.discard)
        pack_ms, lag_ms = eng.last_autocorr_ms()
        rows.append((pick_ms, replay_ms, pack_ms, lag_ms))
        print(json.dumps({"call": k, "pick_ms": pick_ms, "replay_ms": replay_ms, "autocorr_pack_ms": pack_ms,
                          "autocorr_lag_ms": lag_ms, "picks": sum(len(p) for p in picks if p is not None),
                          "tau": ac["tau"], "baseline": ac["baseline"], "n_changeable": int(ac["changeable"].sum())}))
    best = [min(r[i] for r in rows) for i in range(4)]
    print(json.dumps({"walkers": a.walkers, "length": a.length, "fold": a.fold, "steps": a.steps, "max_lag": a.max_lag,
                      "discard": a.discard, "window": a.window, "run_kernel_ms": run_ms, "min_pick_ms": best[0],
                      "min_replay_ms": best[1], "min_autocorr_pack_ms": best[2], "min_autocorr_lag_ms": best[3],
                      "lag_over_pick": best[3] / best[0] if best[0] > 0 else None,
                      "pooled_at": {str(k): float(ac["pooled"][k]) for k in (1, 10, 50, 100, 250, a.max_lag)
                                    if k <= a.max_lag}}))


if __name__ == "__main__":
    main()
