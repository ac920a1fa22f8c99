#!/usr/bin/env python3
"""The kernels of a PPO minibatch step from a rocprofv3 kernel trace of tools/train_timing.py with
--fused-opt (profiles/update_kernel_split.txt):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tt -- \
        python tools/train_timing.py --graph --fused-gru --fused-policy --fused-loss --fused-opt --updates 2
    python tools/update_kernel_split.py DIR OUT.txt

A minibatch step is the run of kernels that ends with k_adam_update; steps whose window also holds a
rollout, GAE or env kernel are left out.  The steps are grouped by their kernel count (the two agent
types differ by one kernel) and the two commonest groups are summarised: kernel time per step by bucket
(scan forward / backward, the narrow layers' weight gradients with --fused-wgrad, the wide layers' with
--fused-wgrad-wide, rocBLAS GEMMs, gathers and copies, loss, optimiser step, rest) and by kernel
name, and the window from the step's first start to its last end.

With --grouped-scan in the traced command the same rule cuts a joint step of all agent types in two: the
kernels up to the first type's k_adam_update (every type's forward, loss and backward, with the grouped
scan launches, and the first type's optimiser step) and the two optimiser kernels of each further type;
the two commonest groups are then those two parts."""
import collections
import csv
import glob
import re
import sys

d, out = sys.argv[1], sys.argv[2]
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
rows = []
for r in csv.DictReader(open(f)):
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
def bucket(n):
    if "k_gru_scan_fwd" in n: return "scan forward"
    if "k_gru_scan_bwd" in n: return "scan backward"
    if "k_xtyw" in n: return "wide weight gradients"
    if "k_xty" in n: return "narrow weight gradients"
    if n.startswith("Cijk_") or "gemm" in n.lower() or "rocblas" in n.lower() or "gemv" in n.lower(): return "rocBLAS GEMMs"
    if "k_moments" in n or "k_loss" in n or "k_final" in n: return "loss"
    if "k_adam" in n: return "optimiser step"
    if re.search(r"index|gather|scatter|copy|Copy|memcpy|cat|Cat", n): return "gathers and copies"
    return "rest"
OUTSIDE = ("k_policy_step", "k_env", "k_gae", "k_split", "k_rollout", "k_book", "k_sample")
steps, cur = [], []
for s, e, n in rows:
    cur.append((s, e, n))
    if "k_adam_update" in n:
        steps.append(cur); cur = []
pure = [w for w in steps if not any(any(o in n for o in OUTSIDE) for _, _, n in w)]
# replayed steps only: the most common kernel count
cnt = collections.Counter(len(w) for w in pure)
with open(out, "w") as o:
    P = lambda *a: print(*a, file=o)
    P(f"trace {f}: {len(rows)} kernels, {len(steps)} minibatch steps, {len(pure)} without rollout/GAE kernels in their window")
    P("kernels per step (count of steps):", dict(cnt.most_common(6)))
    names_all = collections.Counter(n for _, _, n in rows)
    P("kernels outside (by name filter):", {k[:60]: v for k, v in names_all.items() if any(o in k for o in OUTSIDE)})
    for klen, _ in cnt.most_common(2):
        ws = [w for w in pure if len(w) == klen]
        P(f"\n== steps of {klen} kernels: {len(ws)} steps")
        tot = collections.defaultdict(float); num = collections.defaultdict(int); byname = collections.defaultdict(float); nname = collections.Counter()
        wall = []
        for w in ws:
            wall.append((max(e for _, e, _ in w) - w[0][0]) / 1e3)
            for s, e, n in w:
                b = bucket(n); tot[b] += (e - s) / 1e3; num[b] += 1; byname[(b, n)] += (e - s) / 1e3; nname[(b, n)] += 1
        wall.sort()
        k = len(ws)
        P(f"window first start .. last end per step, us: median {wall[k // 2]:.1f}, min {wall[0]:.1f}, max {wall[-1]:.1f}")
        allk = sum(tot.values()) / k
        P(f"sum of kernel times per step: {allk:.1f} us")
        for b in sorted(tot, key=lambda b: -tot[b]):
            P(f"  {b:24s} {tot[b] / k:9.1f} us  {100 * tot[b] / k / allk:5.1f} %  {num[b] / k:6.1f} kernels")
        P("by kernel name (us per step, launches per step):")
        for (b, n), t in sorted(byname.items(), key=lambda x: -x[1])[:45]:
            P(f"  {t / k:9.2f} {nname[(b, n)] / k:6.1f}  [{b}] {n[:110]}")
