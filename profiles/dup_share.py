#!/usr/bin/env python3
"""How many candidates of a random optimizer call repeat a colour that occurred earlier in the call's list.

The generator of gen_candidates / gen_candidates_body restated in numpy (no GPU needed): the key of a call is
mix64(seed ^ step_id * 0x9E3779B97F4A7C15 ^ 0xD1B54A32D192ED03), candidate k takes the low 15 bits of
mix64(key + (k + 1) * 0x9E3779B97F4A7C15).  Defaults are the benchmark's own lists (seed 1, step ids 10..409).

    python profiles/dup_share.py [--seed 1] [--first 10] [--calls 400] [--sizes 64,1024,2048,4096,8192]
"""
import argparse

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def colours(seed, step_id, n):
    with np.errstate(over="ignore"):
        key = mix64(np.uint64(seed) ^ (np.uint64(step_id) * GOLDEN) ^ np.uint64(0xD1B54A32D192ED03))
        return (mix64(key + (np.arange(n, dtype=np.uint64) + np.uint64(1)) * GOLDEN) & np.uint64(32767)).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--first", type=int, default=10)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--sizes", default="64,1024,2048,4096,8192")
    a = ap.parse_args()
    print("| candidates per call | duplicates, mean over %d calls | share | min..max | expected n - 32768 (1 - exp(-n / 32768)) |" % a.calls)
    print("|---|---|---|---|---|")
    for n in (int(v) for v in a.sizes.split(",")):
        d = np.array([n - np.unique(colours(a.seed, a.first + i, n)).size for i in range(a.calls)])
        print("| %d | %.1f | %.2f %% | %d..%d | %.1f |" % (n, d.mean(), 100.0 * d.mean() / n, d.min(), d.max(), n - 32768 * (1 - np.exp(-n / 32768.0))))


if __name__ == "__main__":
    main()
