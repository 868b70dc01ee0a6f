"""The host side of Engine.rollout_lpg (LPG's gradient projection on the device path): the sixth library's device code
and argument checks (its build identity and ABI: tests/test_build_identity.py), the float64 gradient at the zero action against torch autograd,
the float32 projection against the float64 one, the batch helper against a numpy restatement of the buffer, and the
sizing of the GPU tests' probe inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lpg64
import usl64


# the bound on a_safe is informative: on at least 90 % of the corrected rows of every probe case it is below
# C_INFORMATIVE (1 + |a_safe|).  Chosen here, on the CPU, from the float64 restatement alone.
C_INFORMATIVE = 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# device code and argument checks (build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lpg_lib():
    from guardx_amd import build, _lpg_native
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    return _lpg_native.load()          # refuses a library whose build id is not the tree's


def test_no_scratch_in_the_device_code(tmp_path):
    """hipcc --offload-arch=gfx950 compiles every kernel of the library (16 step kernels, 4 probe kernels, the
    transpose) without scratch memory and within the 168 registers that 12 waves per workgroup leave a lane"""
    import subprocess
    from guardx_amd import build
    asm = tmp_path / "gx_lpg.s"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_lpg.hip")])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    print("lpg kernels:", len(scratch), "max vgpr", max(vgpr))
    assert len(scratch) == 21 and max(scratch) == 0 and max(vgpr) <= 168


def test_sizes_and_bad_arguments_are_errors_not_crashes(lpg_lib):
    from guardx_amd import _lpg_native as n
    from guardx_amd.usl import policy_floats, q_floats
    lib = lpg_lib
    for D, A in ((43, 2), (64, 8), (70, 10)):
        Dp = (D + 3) // 4 * 4
        for h in (64, 128, 192, 256):
            assert lib.gxp_params_floats(D, A, h) == policy_floats(D, A, h)
            assert lib.gxp_q_floats(D, A, h) == q_floats(D, A, h)
            assert lib.gxp_probe_work_floats(D, A, h) == Dp * h + h * h
            for hc in (64, 256):
                assert lib.gxp_work_floats(D, A, h, hc) == 2 * (Dp * h + h * h) + Dp * hc + hc * hc
    assert lib.gxp_params_floats(43, 2, 96) == -1 and lib.gxp_q_floats(0, 2, 64) == -1
    assert lib.gxp_q_floats(43, 3, 64) == -1 and lib.gxp_work_floats(43, 2, 64, 32) == -1
    assert lib.gxp_probe_work_floats(43, 18, 64) == -1
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call
    assert lib.gxp_prepare(43, 2, 64, 64, None, fake, fake, None) == n.GXP_ERR_ARG
    assert lib.gxp_prepare(43, 2, 64, 96, fake, fake, fake, None) == n.GXP_ERR_UNSUPPORTED
    assert lib.gxp_prepare(9000, 2, 256, 256, fake, fake, fake, None) == n.GXP_ERR_UNSUPPORTED

    def probe(n_=4, D=43, A=2, hc=64, cp=fake, qi=fake):
        return lib.gxp_projection_probe(n_, D, A, hc, cp, fake, fake, fake, qi, 0.0, 1.0, 1.0, fake, fake, fake, fake,
                                        fake, None)
    assert probe(cp=None) == n.GXP_ERR_ARG and probe(qi=None) == n.GXP_ERR_ARG and probe(n_=-1) == n.GXP_ERR_ARG
    assert probe(hc=96) == n.GXP_ERR_UNSUPPORTED and probe(A=3) == n.GXP_ERR_UNSUPPORTED and probe(A=18) == n.GXP_ERR_UNSUPPORTED
    assert probe(n_=0) == n.GXP_OK

    def args(**over):
        a = n.GxpStepArgs()
        a.struct_size = C.sizeof(n.GxpStepArgs)
        a.N, a.D, a.A, a.hidden, a.c_hidden, a.T, a.t = 4, 43, 2, 64, 64, 3, 1
        for f, _ in n.GxpStepArgs._fields_:
            if f.startswith("d_"):
                setattr(a, f, fake)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.gxp_policy_step(None, None) == n.GXP_ERR_ARG
    assert lib.gxp_policy_step(C.byref(args(struct_size=8)), None) == n.GXP_ERR_ARG
    assert b"struct_size" in lib.gxp_last_error()
    for bad in (dict(N=-1), dict(t=-1), dict(t=4), dict(T=0), dict(d_params=None), dict(d_c_params=None),
                dict(d_cost_in=None), dict(d_act_safe=None), dict(d_qc=None), dict(d_lam=None), dict(d_q_init=None),
                dict(t=3, d_val_last=None), dict(t=0, d_obs0=None)):
        assert lib.gxp_policy_step(C.byref(args(**bad)), None) == n.GXP_ERR_ARG, bad
    for bad in (dict(hidden=96), dict(c_hidden=0), dict(A=3), dict(A=18), dict(D=9000, hidden=256, c_hidden=256)):
        assert lib.gxp_policy_step(C.byref(args(**bad)), None) == n.GXP_ERR_UNSUPPORTED, bad
    assert lib.gxp_policy_step(C.byref(args(N=0)), None) == n.GXP_OK          # N == 0: nothing to do


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement against torch autograd, and the float32 projection against it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["point64", "ant256", "walker128", "saturated192", "threshold20"])
def test_zero_action_gradient_equals_torch_autograd_in_float64(name):
    """probe64's G at grad_scale = 1 is N times the act_0.grad of lpg_core.py:174-178 (pred_0.mean().backward())"""
    import test_gpu_lpg as tg
    qm, obs, act, q_init, delta = tg.probe_inputs(name)
    obs, act = obs[:400], act[:400]
    G = lpg64.probe64(usl64.QCritic(qm), obs, act, q_init[:400], delta, 1.0)['G']
    want = lpg64.torch_autograd_G(qm, obs, act.shape[1])
    scale = np.abs(want).max()
    assert scale > 1e-6 and np.abs(G - want).max() <= 1e-11 * scale, np.abs(G - want).max()
    # the reference's own scale: grad_scale = 1 / N is act_0.grad itself
    Gn = lpg64.probe64(usl64.QCritic(qm), obs, act, q_init[:400], delta, 1.0 / 400)['G']
    np.testing.assert_allclose(Gn, want * float(np.float32(1.0 / 400)), rtol=1e-10, atol=0)


def test_project32_against_the_float64_projection():
    """project32 on exact float32 G and q within project64's own bound (dG = dq = 0: the roundings of the projection
    alone), for both signs; its branches; and its fixed points"""
    rng = np.random.default_rng(3)
    f = np.float32
    for A in (2, 8, 16):
        n = 20000
        G = (rng.normal(size=(n, A)) * rng.choice([1e-4, 1e-2, 1.0, 50.0], size=(n, 1))).astype(f)
        a = (rng.normal(size=(n, A)) * 0.7).astype(f)
        q = rng.random(n).astype(f)
        qi = (0.4 + 0.05 * rng.normal(size=n)).astype(f)
        for sign in (1.0, -1.0):
            got, lam, branch = lpg64.project32(a, G, q, qi, 0.4, sign)
            w = lpg64.project64(a, G, np.zeros_like(G), q, np.zeros(n), qi, 0.4, sign)
            ok = ~w['edge']
            assert w['edge'].mean() < 1e-3
            np.testing.assert_array_equal(branch[ok], w['branch'][ok])
            assert (np.abs(got - w['a_safe'])[ok] <= w['da_safe'][ok]).all()
            assert (np.abs(lam - w['lam'])[ok] <= w['dlam'][ok]).all()
            assert {0, 1, 2} == set(np.unique(branch))
    one = lambda x: np.array([x], f)   # noqa: E731
    # q <= delta keeps the action; G . a == eps gives lam = 0; lam = (G . a - eps) / G . G otherwise
    a_safe, lam, br = lpg64.project32(one([0.5, 0.25]), one([2.0, 0.0]), one(0.3), one(0.0), 0.3)
    assert br[0] == 0 and lam[0] == 0 and (a_safe == one([0.5, 0.25])).all()
    a_safe, lam, br = lpg64.project32(one([0.5, 0.25]), one([2.0, 0.0]), one(0.5), one(0.0), 0.25)
    assert br[0] == 1 and lam[0] == f(0.1875) and (a_safe == one([0.875, 0.25])).all()      # (1 - 0.25) / 4
    a_safe, lam, br = lpg64.project32(one([0.5, 0.25]), one([2.0, 0.0]), one(0.5), one(0.0), 0.25, -1.0)
    assert (a_safe == one([0.125, 0.25])).all()
    a_safe, lam, br = lpg64.project32(one([0.5, 0.25]), one([0.0, 0.0]), one(0.5), one(0.0), 0.25)
    assert br[0] == 2 and lam[0] == 0 and (a_safe == one([0.5, 0.25])).all()                # -eps / 0 = -inf
    a_safe, lam, br = lpg64.project32(one([0.5, 0.25]), one([0.0, 0.0]), one(0.5), one(0.25), 0.25)
    assert br[0] == 2 and np.isnan(lam[0]) and np.isnan(a_safe).all()                       # 0 / 0


# ---------------------------------------------------------------------------------------------------------------------
# the batch helper: LPGBufferX (safe_rl_libX/lpg/lpg.py:26-159) is USLBufferX under another name, so its numpy
# restatement is tests/test_usl_host.py:USLBufferNP
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_done", [False, True])
def test_lpg_rollout_batch_against_the_buffer_restatement(no_done):
    import torch
    from guardx_amd.rollout_buffer import lpg_rollout_batch, usl_rollout_batch
    from test_usl_host import _synthetic, usl_batch_np
    T, N, D, A = 30, 9, 5, 4
    g = _synthetic(T, N, D, A, 6, no_done)
    g['lam'] = np.zeros((T, N), np.float32)
    want = usl_batch_np(g)
    got = lpg_rollout_batch({k: torch.from_numpy(v) for k, v in g.items()})
    assert set(got) == set(want) == {'obs', 'act', 'act_safe', 'ret', 'adv', 'logp', 'mu', 'logstd', 'cost', 'targetc'}
    for k in want:
        tol = 2e-4 if k == 'adv' else 2e-5
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=tol, atol=tol, err_msg=k)
    tc = got['targetc'].numpy().reshape(N, T)
    for e in range(N):
        for t in range(T):
            end = t == T - 1 or g['done'][t, e] > 0
            exp = g['cost'][t, e] + (0.0 if end else np.float32(0.99) * g['qc'][t + 1, e])
            assert abs(tc[e, t] - exp) <= 1e-6
    with pytest.raises(KeyError, match=r"lpg_rollout_batch needs out\['qc'\] \(Engine.rollout_lpg\)"):
        lpg_rollout_batch({k: torch.from_numpy(v) for k, v in g.items() if k != 'qc'})
    with pytest.raises(KeyError, match=r"usl_rollout_batch needs out\['qc'\] \(Engine.rollout_usl\)"):
        usl_rollout_batch({k: torch.from_numpy(v) for k, v in g.items() if k != 'qc'})


# ---------------------------------------------------------------------------------------------------------------------
# sizing the GPU tests' probe inputs with the float64 checker alone
# ---------------------------------------------------------------------------------------------------------------------
def test_probe_inputs_are_sized():
    """On exactly the inputs of tests/test_gpu_lpg.py (probe_inputs), with the float64 restatement alone: every case has
    at least 20 % of its rows in each of the three branches, at most 2 % edge rows (the cap of the GPU test), and an
    informative bound: bound(a_safe) <= C_INFORMATIVE (1 + |a_safe|) on at least 90 % of the corrected rows."""
    import test_gpu_lpg as tg
    for name in sorted(tg.PROBE_CASES):
        qm, obs, act, q_init, delta = tg.probe_inputs(name)
        w = lpg64.probe64(usl64.QCritic(qm), obs, act, q_init, delta, 1.0)
        shares = np.array([(w['branch'] == k).mean() for k in range(3)])
        edge = float(w['edge'].mean())
        corr = w['branch'] == 1
        rel = (w['da_safe'] / (1.0 + np.abs(w['a_safe']))).max(-1)[corr]
        informative = float((rel <= C_INFORMATIVE).mean())
        print(f"lpg sizing {name}: delta {delta:.4f}  branch 0/1/2 {shares[0]:.3f} {shares[1]:.3f} {shares[2]:.3f}  "
              f"edge {edge:.4f}  informative {informative:.3f}  median rel bound {np.median(rel):.2e}  "
              f"median |G| {np.median(np.abs(w['G'])):.2e}")
        assert (shares >= 0.2).all(), (name, shares)
        assert edge <= tg.EDGE_CAP, (name, edge)
        assert np.isfinite(w['dq']).all() and np.isfinite(w['dG']).all()
        assert informative >= 0.9, (name, informative)
