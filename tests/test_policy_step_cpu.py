"""The fused policy step without a GPU: the C-ABI surface of hftlob_policy_step (declared, exported,
argument checks before any device call), the torch restatement against ActorCriticRNN.step, the
host-side Gumbel noise, the size rule, the learner's FUSED_POLICY switch and the evaluation
script's argument parser."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from hftlob import _lib
from hftlob import evaluate as EV
from hftlob.train import ippo as I
from hftlob.train import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hftlob.h")


def assert_close(name, got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert not got.any(), f"{name}: reference is 0 everywhere, got max |x| = {float(got.abs().max())}"
        return
    worst = float(((got - ref).abs() / (1e-5 * ref.abs() + 1e-5 * scale)).max())
    assert worst <= 1.0, f"{name}: max error / bound = {worst}"


def test_abi_surface():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(hftlob_[a-z_]+)\s*\(", src))
    assert "hftlob_policy_step" in declared and "hftlob_policy_step" in _lib.EXPORTS
    assert re.search(r"\}\s*hftlob_policy_weights\s*;", src)
    for name in P.WEIGHT_NAMES:
        assert re.search(r"\*\s*" + name + r"\b", src), name
    assert [n for n, _ in _lib.PolicyWeights._fields_] == list(P.WEIGHT_NAMES)
    assert C.sizeof(_lib.PolicyWeights) == 14 * C.sizeof(C.c_void_p)
    assert "ippo_rnn_JAXMARL.py:53-78, 183-256" in src
    assert _lib.ABI_VERSION == 8 and "#define HFTLOB_ABI_VERSION 8" in src
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "hftlob_policy_step" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_argument_checks_run_before_any_device_call():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libhftlob.so not built (run __graft_entry__.build())")
    L = _lib.lib()
    k = C.c_void_p(64)   # never dereferenced: the checks run on the host before any device call
    ws = _lib.PolicyWeights(*([64] * 14))
    EINVAL, ENULL, ESHAPE = -1, -2, -3

    def call(B=8, D=6, FC=64, H=64, A=5, w=C.byref(ws), obs=k, done=k, h_in=k, h_out=k, mode=1, key=None, action=k,
             log_prob=k, value=k, logits=None):
        return L.hftlob_policy_step(B, D, FC, H, A, w, obs, done, h_in, h_out, mode, key, action, log_prob, value,
                                    logits, None)

    for kw, code, word in ((dict(H=96), ESHAPE, b"H"), (dict(H=32), ESHAPE, b"H"), (dict(FC=512), ESHAPE, b"FC"),
                           (dict(A=17), ESHAPE, b"A"), (dict(A=0), ESHAPE, b"A"), (dict(D=0), ESHAPE, b"D"),
                           (dict(D=65), ESHAPE, b"D"), (dict(B=0), ESHAPE, b"B"), (dict(mode=2), EINVAL, b"mode"),
                           (dict(mode=-1), EINVAL, b"mode"), (dict(obs=None), ENULL, b"obs"),
                           (dict(done=None), ENULL, b"done"), (dict(h_in=None), ENULL, b"h_in"),
                           (dict(h_out=None), ENULL, b"h_out"), (dict(mode=0, key=None), ENULL, b"key"),
                           (dict(action=None), ENULL, b"action"), (dict(log_prob=None), ENULL, b"log_prob"),
                           (dict(value=None), ENULL, b"value"), (dict(w=None), ENULL, b"w")):
        assert call(**kw) == code, kw
        assert word in L.hftlob_last_error(), (kw, L.hftlob_last_error())
    for name in P.WEIGHT_NAMES:                     # every pointer of the struct is required
        bad = _lib.PolicyWeights(*([64] * 14))
        setattr(bad, name, None)
        assert call(w=C.byref(bad)) == ENULL, name
    bad = _lib.PolicyWeights(*([64] * 14))
    bad.w_hh = 68                                   # float4 reads: the matrices the kernel streams are 16-byte aligned
    assert call(w=C.byref(bad)) == EINVAL and b"aligned" in L.hftlob_last_error()
    with pytest.raises(RuntimeError, match="device"):   # a CPU tensor raises through _lib.ptr
        net = I.ActorCriticRNN(6, 5, 64, 64)
        P.policy_step(net, torch.zeros(4, 6), torch.zeros(4, dtype=torch.bool), torch.zeros(4, 64), 1)


@pytest.mark.parametrize("B,D,FC,H,A", [(1, 3, 16, 8, 2), (9, 6, 64, 64, 5), (17, 13, 32, 64, 16)])
def test_reference_matches_the_module_step(B, D, FC, H, A):
    torch.manual_seed(B)
    net = I.ActorCriticRNN(D, A, FC, H)
    with torch.no_grad():
        for p in net.parameters():                  # non-zero biases, a head with a real logit range
            if p.dim() == 1:
                p.copy_(0.3 * torch.randn_like(p))
        net.actor2.weight.mul_(100.0)
    obs, h = torch.randn(B, D), torch.randn(B, H)
    done = torch.arange(B) % 2 == 1
    with torch.no_grad():
        h1, logits, v = net.step(h, obs, done)
        logp = torch.log_softmax(logits, -1)
    rh, rl, rv, ra, rlp = P.policy_step_reference(net, obs, done, h, P.GREEDY)
    assert rl.dtype == torch.float32 and ra.dtype == torch.int64
    assert_close("h", rh, h1)
    assert_close("logits", rl, logits)
    assert_close("value", rv, v)
    assert torch.equal(ra, rl.argmax(-1))
    assert_close("log_prob", rlp, logp.gather(-1, ra[:, None]).squeeze(-1))
    # mode 0: the given noise decides; a key gives gumbel_noise(key)
    g = torch.zeros(B, A)
    g[:, A - 1] = 1e3
    assert bool((P.policy_step_reference(net, obs, done, h, P.SAMPLE, gumbel=g)[3] == A - 1).all())
    key = np.array([0, 11], np.uint32)
    a_key = P.policy_step_reference(net, obs, done, h, P.SAMPLE, key=key)[3]
    assert torch.equal(a_key, (rl + P.gumbel_noise(key, B, A)).argmax(-1))
    with pytest.raises(ValueError):
        P.policy_step_reference(net, obs, done, h, P.SAMPLE)
    # float64 in, float64 out
    assert P.policy_step_reference(net, obs.double(), done, h.double(), P.GREEDY)[1].dtype == torch.float64


def test_first_argmax_on_ties():
    W = {k: v.detach().clone() for k, v in P.net_weights(I.ActorCriticRNN(4, 6, 16, 8)).items()}
    W["w_a2"].zero_()
    W["b_a2"].copy_(torch.tensor([0.0, 2.0, 1.0, 2.0, -1.0, 2.0]))
    a = P.policy_step_reference(W, torch.randn(5, 4), torch.zeros(5, dtype=torch.bool), torch.randn(5, 8), P.GREEDY)[3]
    assert a.tolist() == [1] * 5


def test_supported_sizes():
    ok = P.policy_step_supported
    assert ok(6, 64, 64, 5) and ok(64, 256, 256, 16) and ok(1, 128, 64, 1)
    assert not ok(6, 63, 64, 5) and not ok(6, 64, 63, 5)
    assert not ok(6, 257, 256, 5) and not ok(6, 256, 257, 5)
    assert not ok(6, 96, 64, 5) and not ok(6, 64, 32, 5)
    assert ok(6, 64, 64, 16) and not ok(6, 64, 64, 17) and not ok(6, 64, 64, 0)
    assert not ok(0, 64, 64, 5) and ok(64, 64, 64, 5) and not ok(65, 64, 64, 5)
    assert P.SUPPORTED_HIDDEN == (64, 128, 256)


def test_gumbel_noise_is_finite_at_the_edges_and_follows_the_formula():
    g = P.gumbel_from_bits(np.array([0, 0xFFFFFFFF, 0x1FF, 0x200], dtype=np.uint32))
    assert g.dtype == np.float32 and np.isfinite(g).all()
    tiny = float(np.finfo(np.float32).tiny)
    assert g[0] == np.float32(-np.log(-np.log(np.float32(tiny))))      # f = 0: the clamp gives u = tiny
    assert g[2] == g[0]                                                 # the low 9 bits are dropped
    assert g[1] == np.float32(-np.log(-np.log(np.float32(1.0 - 2.0 ** -23))))
    n = P.gumbel_noise(np.array([0, 3], np.uint32), 7, 5)
    assert n.shape == (7, 5) and n.dtype == torch.float32 and bool(torch.isfinite(n).all())
    # element (b, a) comes from counter b A + a: a longer draw with the same A starts with the same rows
    assert torch.equal(P.gumbel_noise(np.array([0, 3], np.uint32), 9, 5)[:7], n)
    assert not torch.equal(P.gumbel_noise(np.array([0, 4], np.uint32), 7, 5), n)
    # a torch key (int32 words, as the device keys are) reads as the same unsigned words
    assert torch.equal(P.gumbel_noise(torch.tensor([0, -2], dtype=torch.int32), 3, 4),
                       P.gumbel_noise(np.array([0, 0xFFFFFFFE], np.uint32), 3, 4))


def test_random_bits_match_the_oracle():
    from oracle import ref_py as R
    for key, n in (((0, 100), 17 * 16), ((123456789, 0xFFFFFFFF), 40)):
        assert P.random_bits(np.array(key, np.uint32), n).tolist() == R.random_bits(key, n, True)


def test_config_switch():
    from test_ippo import FakeEnv
    assert I.default_config()["FUSED_POLICY"] is False
    kw = dict(NUM_ENVS=16, NUM_STEPS=4, FC_DIM_SIZE=64, GRU_HIDDEN_DIM=64, NUM_MINIBATCHES=2, UPDATE_EPOCHS=1,
              TOTAL_TIMESTEPS=16 * 4 * 4, SEED=0)
    with pytest.raises(ValueError, match="FUSED_POLICY needs a GPU device"):
        I.IPPOTrainer(FakeEnv(), I.default_config(FUSED_POLICY=True, **kw), device="cpu")
    off = I.IPPOTrainer(FakeEnv(), I.default_config(**kw), device="cpu")
    assert off.fused_policy is False and not hasattr(off, "pol_rng")


def test_checkpoint_round_trip_on_the_cpu(tmp_path):
    from test_ippo import FakeEnv
    kw = dict(NUM_ENVS=16, NUM_STEPS=4, FC_DIM_SIZE=16, GRU_HIDDEN_DIM=16, NUM_MINIBATCHES=2, UPDATE_EPOCHS=1,
              TOTAL_TIMESTEPS=16 * 4 * 4, SEED=0)
    a = I.IPPOTrainer(FakeEnv(), I.default_config(**kw), device="cpu")
    a.update()
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path)
    b = I.IPPOTrainer(FakeEnv(), I.default_config(**dict(kw, SEED=5)), device="cpu")
    b.load_checkpoint(path)
    assert b.opt_count == a.opt_count and a.opt_count[0] > 0
    for na, nb, oa, ob in zip(a.nets, b.nets, a.opts, b.opts):
        for (k, x), (_, y) in zip(na.state_dict().items(), nb.state_dict().items()):
            assert torch.equal(x, y), k
        sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
        assert sa.keys() == sb.keys() and len(sa) > 0
        for p in sa:
            for k in sa[p]:
                assert torch.equal(torch.as_tensor(sa[p][k]), torch.as_tensor(sb[p][k])), (p, k)
    nets = I.load_policy(path, device="cpu")
    for na, n in zip(a.nets, nets):
        assert all(torch.equal(x, y) for x, y in zip(na.state_dict().values(), n.state_dict().values()))
    b.update()                                      # the restored trainer goes on training
    with pytest.raises(ValueError, match="not an IPPOTrainer checkpoint"):
        torch.save({"nets": []}, str(tmp_path / "other.pt"))
        I.load_policy(str(tmp_path / "other.pt"))


def test_evaluate_parser_takes_exactly_one_of_the_two():
    ap = EV.build_parser()
    base = ["--env-config", "2_player_fq_fqc", "--envs", "4", "--steps", "5"]
    a = ap.parse_args(base + ["--fixed-actions", "0,1"])
    assert a.fixed_actions == "0,1" and a.checkpoint is None and a.sample is False
    b = ap.parse_args(base + ["--checkpoint", "x.pt", "--sample"])
    assert b.checkpoint == "x.pt" and b.fixed_actions is None and b.sample is True
    assert ap.parse_args(base + ["--checkpoint", "x.pt"]).sample is False
    for extra in ([], ["--fixed-actions", "0,1", "--checkpoint", "x.pt"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + extra)


def test_evaluate_policy_needs_the_info_words():
    class NoInfo:
        return_info = False
    with pytest.raises(ValueError, match="return_info=True"):
        EV.evaluate_policy(NoInfo(), [], 4, 4, 0)
