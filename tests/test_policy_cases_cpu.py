"""The conditions that the fixtures of tests/policy_cases.py must meet on their own, without a GPU:
exact action comparison is sound (top-two gap), the tolerance keeps a 4x margin over what float32
needs, the saturated cases are saturated, and every instantiation of csrc/policy_step.hip has a
case.  These are conditions on the inputs, not measurements of the kernel."""
import pytest
import torch

import policy_cases as PC
from hftlob.train import policy as P


def test_the_case_list_names_every_instantiation():
    """The (FC, H) pairs come from the kernel's own HFTLOB_POLICY_CASE lines: an instantiation added
    there has no case, and fails here, until the list names it."""
    pairs = PC.kernel_pairs()
    assert len(pairs) == len(set(pairs)) == 9, pairs
    assert pairs == sorted(PC.PAIRS)
    for kind in ("full", "ragged"):
        assert sorted((fc, h) for k, fc, h in PC.CASES if k == kind) == pairs, kind
    assert [(fc, h) for k, fc, h in PC.CASES if k == "saturated"] == PC.SATURATED_PAIRS
    assert set(PC.SATURATED_PAIRS) <= set(pairs) and len(set(PC.CASES)) == len(PC.CASES)
    for (B, D, nvec, _, _), (FC, H) in ((PC.KINDS[k], (fc, h)) for k, fc, h in PC.CASES):
        assert P.policy_step_multi_supported(D, FC, H, nvec) and B % 16 != 0
    assert all(set(P.SUPPORTED_HIDDEN) == {x[i] for x in pairs} for i in (0, 1))


def test_scale_one_is_the_multi_head_tests_recipe():
    """The draw order of make_case: at scale 1 the weights and the reference are those of a direct
    restatement with the same seed."""
    B, D, FC, H, nvec, seed = 5, 7, 64, 128, (3, 2), 9
    W, x, ref, info = PC.make_case(B, D, FC, H, nvec, "odd", 1.0, seed)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    for name, o, i in (("embed", FC, D), ("ih", 3 * H, FC), ("hh", 3 * H, H), ("c1", FC, H), ("c2", 1, FC),
                       ("a1", H, H), ("a2", sum(nvec), H)):
        assert torch.equal(W["w_" + name], r(o, i) / i ** 0.5) and torch.equal(W["b_" + name], 0.5 * r(o)), name
        assert W["w_" + name].dtype == torch.float32 and bool(W["b_" + name].any())
    assert torch.equal(x["obs"], r(B, D)) and torch.equal(x["h"], r(B, H))
    assert x["done"].tolist() == [False, True, False, True, False]
    assert ref["h"].dtype == torch.float64 and ref["action"].shape == (B, 2) and info["seed"] == seed
    W4, x4, _, _ = PC.make_case(B, D, FC, H, nvec, "odd", 4.0, seed)
    for name in W:
        assert torch.equal(W4[name], W[name] * (4.0 if name in ("w_ih", "w_hh", "b_ih") else 1.0)), name
    assert torch.equal(x4["obs"], 4.0 * x["obs"]) and torch.equal(x4["h"], x["h"])


@pytest.mark.parametrize("c", PC.CASES, ids=PC.case_id)
def test_fixture_conditions(c):
    kind, FC, H = c
    B, D, nvec, W, x, ref, info = PC.named_case(*c)
    share = info["share"]
    print(f"{PC.case_id(c)}: seed {info['seed']}, top-two gap {info['gap']:.3e}, float32 CPU share of the bound: "
          + ", ".join(f"{k} {v:.4f}" for k, v in share.items()))
    assert info["seed"] in range(64) and info["gap"] >= PC.GAP
    assert share["max"] <= 0.25                                        # the bound keeps 4x over what float32 needs
    assert tuple(x["obs"].shape) == (B, D) and tuple(ref["logits"].shape) == (B, sum(nvec))
    if kind == "saturated":
        frac = float((ref["h"].abs() > 0.999).double().mean())
        print(f"share of |h_ref| > 0.999 = {frac:.3f}")
        assert frac >= 0.20
