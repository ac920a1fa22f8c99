"""The policy step's test cases, shared by tests/test_gpu_policy_shapes.py and
tests/test_policy_cases_cpu.py: one generator of float32 weights and inputs with their float64
reference, and the list of cases that launches every (FC, H) instantiation of
csrc/policy_step.hip at the edges of its shapes.

The project's tolerance, per tensor, is |got - ref| <= 1e-5 |ref| + 1e-5 max|ref|.  Next to the
reference a case carries two figures computed on the CPU, conditions on the fixture and not
measurements of a kernel: the smallest float64 top-two logit gap over rows and heads (actions are
compared exactly, which is sound only where it is far above a float32 sum's error of about 1e-6),
and the share of the tolerance that the float32 CPU restatement of the same operator uses."""
import functools
import os
import re

import torch

from hftlob.train import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "jaxmarl-hft_amd", "csrc", "policy_step.hip")

GAP = 1e-3
SIZES = (64, 128, 256)
PAIRS = [(FC, H) for FC in SIZES for H in SIZES]                       # (FC, H), every instantiation
SATURATED_PAIRS = [(64, 256), (256, 64), (128, 128)]

# kind: (B, D, nvec, done pattern, scale)
#   full       two tiles and one live row; no obs column is padding, and at H = 64 the obs tile covers
#              the whole buffer that h is written into; a full logits block; done on the odd rows
#   ragged     the second tile has one live row; the k < D mask cuts inside the last MFMA k-group; a dead
#              logits lane in every head, a one-logit head, an offset that is no multiple of 4
#   saturated  w_ih, w_hh, b_ih and obs times 4: a good part of the gates is 0 or 1 in float32
KINDS = {"full": (33, 64, (16,), "odd", 1.0), "ragged": (17, 61, (3, 16, 1, 5), "odd", 1.0),
         "saturated": (18, 61, (7,), "odd", 4.0)}
CASES = ([("full", FC, H) for FC, H in PAIRS] + [("ragged", FC, H) for FC, H in PAIRS]
         + [("saturated", FC, H) for FC, H in SATURATED_PAIRS])


def case_id(c):
    return f"{c[0]}-FC{c[1]}-H{c[2]}"


def kernel_pairs():
    """The (FC, H) pairs csrc/policy_step.hip instantiates: its HFTLOB_POLICY_CASE(h, fc) lines."""
    with open(KERNEL) as f:
        found = re.findall(r"^\s*HFTLOB_POLICY_CASE\(\s*(\d+)\s*,\s*(\d+)\s*\)", f.read(), re.M)
    return sorted((int(fc), int(h)) for h, fc in found)


def bound_share(got, ref):
    """max |got - ref| / (1e-5 |ref| + 1e-5 max|ref|): the share of the tolerance that got uses."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * scale)).max())


def heads_gap(score, nvec):
    """The smallest float64 top-two gap over every row of every head (a one-logit head has no second)."""
    gaps = [float("inf")]
    for s in score.double().split(list(nvec), -1):
        if s.shape[-1] > 1:
            top = s.topk(2, dim=-1).values
            gaps.append(float((top[:, 0] - top[:, 1]).min()))
    return min(gaps)


def done_rows(B, pattern):
    if pattern not in ("odd", "all", "none"):
        raise ValueError(f"done pattern {pattern!r}")
    return {"odd": torch.arange(B) % 2 == 1, "all": torch.ones(B, dtype=torch.bool),
            "none": torch.zeros(B, dtype=torch.bool)}[pattern]


def make_case(B, D, FC, H, nvec, done, scale, seed):
    """Float32 weights (randn / sqrt(fan_in), biases 0.5 randn, w_a2 at gain 1) and inputs, drawn in
    the order of tests/test_gpu_policy_multi.py's make_case, then w_ih, w_hh, b_ih and obs times
    ``scale``; the float64 reference of mode 1 from those float32 values; and the fixture's figures:
    ``gap`` (heads_gap of the reference logits) and ``share`` (bound_share of the float32 CPU
    restatement per tensor, and their largest as ``share["max"]``)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    lin = lambda o, i: (r(o, i) / i ** 0.5, 0.5 * r(o))  # noqa: E731
    W = {}
    for name, o, i in (("embed", FC, D), ("ih", 3 * H, FC), ("hh", 3 * H, H), ("c1", FC, H), ("c2", 1, FC),
                       ("a1", H, H), ("a2", sum(nvec), H)):
        W["w_" + name], W["b_" + name] = lin(o, i)
    x = dict(obs=r(B, D), h=r(B, H), done=done_rows(B, done))
    if scale != 1.0:
        for name in ("w_ih", "w_hh", "b_ih"):
            W[name] = W[name] * scale
        x["obs"] = x["obs"] * scale
    names = ("h", "logits", "value", "action", "log_prob")
    ref = dict(zip(names, P.policy_step_multi_reference({k: v.double() for k, v in W.items()}, x["obs"].double(),
                                                        x["done"], x["h"].double(), P.GREEDY, nvec)))
    f32 = dict(zip(names, P.policy_step_multi_reference(W, x["obs"], x["done"], x["h"], P.GREEDY, nvec)))
    share = {k: bound_share(f32[k], ref[k]) for k in ("h", "logits", "value", "log_prob")}
    share["max"] = max(share.values())
    return W, x, ref, dict(gap=heads_gap(ref["logits"], nvec), share=share, seed=seed)


@functools.lru_cache(maxsize=None)
def case(B, D, FC, H, nvec, done, scale):
    """make_case at the first seed of range(64) whose gap reaches GAP; computed once per shape and not
    modified by the tests."""
    for seed in range(64):
        out = make_case(B, D, FC, H, nvec, done, scale, seed)
        if out[3]["gap"] >= GAP:
            return out
    raise AssertionError(f"no seed in range(64) gives a top-two gap >= {GAP}")


def named_case(kind, FC, H, done=None):
    """The case of the list (W, x, ref, info), with its sizes (B, D, nvec) in front; ``done`` replaces
    the kind's done pattern."""
    B, D, nvec, pattern, scale = KINDS[kind]
    return (B, D, nvec) + case(B, D, FC, H, nvec, done or pattern, scale)
