"""The grouped policy step without a GPU: the header's declaration and the ctypes mirror, the config default,
the per-group reference (the operator's spec) against the single references, and the support check at its
edges."""
import ctypes as C
import os
import re

import pytest
import torch

import policy_cases as PC
from hftlob import _lib
from hftlob.train import ippo as I
from hftlob.train import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "hftlob.h")) as f:
    HEADER = f.read()


def test_header_declares_the_entry_point_and_the_struct():
    assert "hftlob_policy_step_grouped" in _lib.EXPORTS
    assert re.search(r"^int hftlob_policy_step_grouped\(int FC, int H, int n_groups, const hftlob_policy_group\* groups",
                     HEADER, re.M)
    assert re.search(r"#define HFTLOB_POLICY_MAX_GROUPS 8\b", HEADER)
    assert P.MAX_GROUPS == 8
    body = re.search(r"typedef struct \{([^}]*)\} hftlob_policy_group;", HEADER).group(1)
    names = re.findall(r"[\s*]([A-Za-z_0-9]+)(?:\[\d+\])?\s*(?:/\*[^*]*\*/)?\s*[,;]", body)
    assert names == [n for n, _ in _lib.PolicyGroup._fields_]
    assert "#define HFTLOB_ABI_VERSION 8" in HEADER and _lib.ABI_VERSION == 8


def test_ctypes_mirror_has_the_c_layout():
    # int B, D, K; int nvec[4]: 28 bytes, padded to the weights' 8-byte alignment; 14 + 9 pointers
    G = _lib.PolicyGroup
    assert G.B.offset == 0 and G.D.offset == 4 and G.K.offset == 8 and G.nvec.offset == 12
    assert G.w.offset == 32 and C.sizeof(_lib.PolicyWeights) == 14 * 8
    assert G.obs.offset == 32 + 14 * 8 and G.logits.offset == 32 + 14 * 8 + 8 * 8
    assert C.sizeof(G) == 32 + 23 * 8


def test_the_switch_is_off_by_default_and_has_a_flag():
    assert I.default_config()["GROUPED_POLICY"] is False
    sw = {s.key: s for s in I.SWITCHES}["GROUPED_POLICY"]
    assert sw.flag == "--grouped-policy" and sw.gpu


def groups():
    """Three groups of one FC and H: a flat head, four heads, one head given as a list."""
    out = []
    for B, D, nvec in ((5, 2, (10,)), (17, 61, (3, 16, 1, 5)), (3, 12, (13,))):
        W, x, _, _ = PC.case(B, D, 64, 128, nvec, "odd", 1.0)
        out.append((W, x, nvec))
    return out


@pytest.mark.parametrize("mode", [P.SAMPLE, P.GREEDY])
def test_reference_is_the_per_group_references(mode):
    gs = groups()
    keys = [torch.tensor([0x1234 + g, 0xABCDEF01 + 7 * g], dtype=torch.int64).to(torch.int32) for g in range(3)]
    heads = [10, [3, 16, 1, 5], [13]]
    got = P.policy_step_grouped_reference([W for W, _, _ in gs], [x["obs"] for _, x, _ in gs],
                                          [x["done"] for _, x, _ in gs], [x["h"] for _, x, _ in gs], mode,
                                          keys=keys if mode == P.SAMPLE else None, heads=heads)
    assert len(got) == 3
    for g, ((W, x, nvec), hd) in enumerate(zip(gs, heads)):
        key = keys[g] if mode == P.SAMPLE else None
        if isinstance(hd, int):
            want = P.policy_step_reference(W, x["obs"], x["done"], x["h"], mode, key=key)
        else:
            want = P.policy_step_multi_reference(W, x["obs"], x["done"], x["h"], mode, nvec, key=key)
        for a, b in zip(got[g], want):
            assert a.shape == b.shape and torch.equal(a, b), g
    assert got[0][3].shape == (5,) and got[2][3].shape == (3, 1)


def test_reference_takes_the_heads_from_a_net():
    torch.manual_seed(0)
    nets = [I.ActorCriticRNN(3, 5, 16, 8), I.ActorCriticRNN(4, [2, 3], 16, 8)]
    obss, hs = [torch.randn(6, 3), torch.randn(4, 4)], [torch.randn(6, 8), torch.randn(4, 8)]
    dones = [torch.zeros(6, dtype=torch.bool), torch.ones(4, dtype=torch.bool)]
    got = P.policy_step_grouped_reference(nets, obss, dones, hs, P.GREEDY)
    assert got[0][3].shape == (6,) and got[1][3].shape == (4, 2)
    want = P.policy_step_multi_reference(nets[1], obss[1], dones[1], hs[1], P.GREEDY, [2, 3])
    assert all(torch.equal(a, b) for a, b in zip(got[1], want))


def test_supported_at_its_edges():
    torch.manual_seed(0)
    net = lambda D=3, A=5, FC=64, H=64: I.ActorCriticRNN(D, A, FC, H)  # noqa: E731
    ok = P.policy_step_grouped_supported
    assert not ok([])
    assert ok([net()]) and ok([net() for _ in range(8)]) and not ok([net() for _ in range(9)])
    assert ok([net(), net(D=64, A=[16, 16, 16, 16], FC=64, H=64)])
    assert not ok([net(), net(FC=128)]) and not ok([net(), net(H=128)])          # one FC and one H
    assert not ok([net(), net(D=65)]) and not ok([net(), net(A=17)]) and not ok([net(), net(A=[2] * 5)])
    assert not ok([net(FC=32, H=32)])
    W = PC.case(5, 2, 64, 128, (10,), "odd", 1.0)[0]
    assert ok([W], heads=[10]) and ok([W], heads=[[4, 6]]) and not ok([W], heads=[[4, 5]])


def test_host_operator_refuses_bad_lists():
    with pytest.raises(ValueError, match="1..8 nets"):
        P.policy_step_grouped([], [], [], [], P.GREEDY)
    with pytest.raises(ValueError, match="one entry per net"):
        P.policy_step_grouped([object()], [], [], [], P.GREEDY)
