"""The layout sampler's chain of kernels (gx_kernels.hip: sample_phase0 -> sample_phase1 -> sample_phase2 -> scan_compact,
pool_export / pool_install for the sharded form) where its index arithmetic is at an edge: the arenas of
tests/layout_np.py -- candidate counts around a wave, a block and a compaction tile, pools of zero to two rows, nearly
every candidate valid, dense arenas whose objects fail all ten tries, margins and thresholds that are no exact floats,
3 to 24 objects (both sides of the four-waves-per-workgroup limit of phase 2, the neighbours of the key tape's object
count), pillars, fixed locations, per-object rectangles, the phase-0 pruning within 1e-4 of its cutoff, shards that
export nothing.  Every case runs in both forms of the sampler, the small ones also under a grid cap of 1 and 3
workgroups, the ones with a key tape also with a tape of 0 and of 37 slots.  Pool size, every pool row, the reset
observation and the layouts handed to the envs equal the CPU checker's bit for bit, on the inline pool of the first
reset and the prefetched pool of the second, and so do the three steps with reset_done that follow each of the two.  tests/test_layout_np.py pins the checker's pools of these arenas to an
independent numpy statement and asserts what each arena is there for."""
import numpy as np
import pytest

import layout_np as ln
from layout_np import CASES, ENV_NUM, NUM_STEPS, SHARDED


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


_CHECKER = {}


def _checker(oracle, case):
    """per reset of the case, the checker's (L, pool, reset observation, objs, steps): `steps` is what each of the
    num_steps zero-action steps with reset_done AFTER that reset returns (their reset_done draws from that reset's
    pool; none after an empty pool, whose envs have no layout).  Computed once per case, read-only"""
    if case.name not in _CHECKER:
        O = oracle.OracleEngine(case.cfg, n_candidates=case.M)
        out = []
        for r in range(case.resets):
            obs = O.reset(check=False)
            rec = [O.layout_size, O.get_pool(), obs, O.get_state()['objs'], []]
            out.append(rec)
            if O.layout_size == 0:
                break
            for _ in range(NUM_STEPS):
                sobs, _, done, _ = O.step(np.zeros((ENV_NUM, 2), np.float32))
                rec[4].append((sobs, done, O.reset_done(), O.get_state()['objs']))
            for a in rec[1:4] + [x for st in rec[4] for x in st]:
                a.setflags(write=False)
        _CHECKER[case.name] = out
    return _CHECKER[case.name]


def _run(torch, oracle, case):
    from guardx_amd import Engine, ResamplingError
    E = Engine(case.cfg, n_candidates=case.M)
    try:
        zero = torch.zeros(ENV_NUM, 2, device='cuda')

        def same_pool_and_layouts(r, L_c, pool_c, objs_c):
            pool = E.get_pool(case.M)
            assert len(pool) == L_c, f"reset {r}: layout_size"
            if L_c:                     # (reset_apply leaves the envs and the observation alone when the pool is empty)
                np.testing.assert_array_equal(pool, pool_c, err_msg=f"reset {r}: pool rows")
                np.testing.assert_array_equal(E.get_state()['objs'], objs_c, err_msg=f"reset {r}: objs")

        for r, (L, pool_c, obs_c, objs_c, steps_c) in enumerate(_checker(oracle, case)):
            obs = E.reset(check=False)
            same_pool_and_layouts(r, L, pool_c, objs_c)
            if L:
                np.testing.assert_array_equal(obs.cpu().numpy(), obs_c, err_msg=f"reset {r}: observation")
            if r == 1:
                assert E.prefetch_stats()[0] == 1       # the second pool was the prefetched one
            if L <= ENV_NUM:
                # every pool too small for the envs is reported with its size.  No step() since the reset: the key, hence
                # the pool and the layouts handed out, are the same again (sampled inline, the prefetch is discarded)
                with pytest.raises(ResamplingError, match=rf"valid layout is {L} <= env_num {ENV_NUM}\b"):
                    E.reset()
                same_pool_and_layouts(r, L, pool_c, objs_c)
            for t, (sobs_c, done_c, rd_c, robjs_c) in enumerate(steps_c):     # reset_done draws from the pool of reset r
                obs, _, done, _ = E.step(zero)
                rd = E.reset_done()
                np.testing.assert_array_equal(obs.cpu().numpy(), sobs_c, err_msg=f"step {t} after reset {r}")
                np.testing.assert_array_equal(done.cpu().numpy(), done_c, err_msg=f"step {t} after reset {r}")
                np.testing.assert_array_equal(rd.cpu().numpy(), rd_c, err_msg=f"reset_done {t} after reset {r}")
                np.testing.assert_array_equal(E.get_state()['objs'], robjs_c, err_msg=f"reset_done {t} after reset {r}")
    finally:
        E.close()


FORMS = ["0", "1"]


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_pool_equals_the_checkers(torch_cuda, oracle, monkeypatch, case, fused):
    """three-phase and fused form (either is valid for any geometry)"""
    monkeypatch.setenv("GX_SAMPLE_FUSED", fused)
    _run(torch_cuda, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["0", "37"])
@pytest.mark.parametrize("case", [c for c in CASES if c.n_tape_objects == 8], ids=repr)
def test_pool_with_a_short_key_tape(torch_cuda, oracle, monkeypatch, case, cap):
    """8 hazards: the three-phase form has a key tape.  No tape slots (every wave walks the chain), and 37 (below that
    many phase-1 survivors one partial wave reads the tape; above, the first wave's survivors have entries it must not use)"""
    monkeypatch.setenv("GX_SAMPLE_FUSED", "0")
    monkeypatch.setenv("GX_SAMPLE_TAPE_CAP", cap)
    _run(torch_cuda, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("case", [c for c in CASES if c.M <= 4097], ids=repr)
def test_pool_under_a_grid_cap(torch_cuda, oracle, monkeypatch, case, grid, fused):
    """phases 1 and 2 on one and on three workgroups: every grid-stride round but the last with whole blocks"""
    monkeypatch.setenv("GX_SAMPLE_FUSED", fused)
    monkeypatch.setenv("GX_SAMPLE_GRID_CAP", grid)
    _run(torch_cuda, oracle, case)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", FORMS)
@pytest.mark.parametrize("case,n_shards", SHARDED, ids=repr)
def test_sharded_pool_equals_the_unsharded(torch_cuda, oracle, monkeypatch, case, n_shards, fused):
    """sample_shard / reset_from_shards with a candidate count the shards do not divide; at M = 257 / 8 some shards
    export no row.  One engine plays every rank in turn."""
    torch = torch_cuda
    from guardx_amd import Engine
    monkeypatch.setenv("GX_SAMPLE_FUSED", fused)
    _, ok = ln.sample_pool(case.cfg, case.key(0), case.M, rows_of_failed=False)
    counts_np = [int(ok[a:b].sum()) for a, b in ln.shard_ranges(case.M, n_shards)]
    L_c, pool_c, obs_c, objs_c, _ = _checker(oracle, case)[0]
    full = Engine(case.cfg, n_candidates=case.M)
    sh = Engine(case.cfg, n_candidates=case.M)
    try:
        sh.set_prefetch(-1)
        o_full = full.reset(check=False)
        parts = [sh.sample_shard(s, n_shards) for s in range(n_shards)]     # (fresh export buffers per call)
        rows_all = torch.stack([p[0] for p in parts])
        counts = torch.cat([p[1] for p in parts])
        assert counts.tolist() == counts_np
        exported = np.concatenate([p[0][:c].cpu().numpy() for p, c in zip(parts, counts_np)])
        pool = full.get_pool(case.M)
        assert len(pool) == L_c == sum(counts_np)
        np.testing.assert_array_equal(exported, pool)
        np.testing.assert_array_equal(pool, pool_c)
        o_sh = sh.reset_from_shards(rows_all, counts, check=False)
        assert torch.equal(o_sh, o_full)
        np.testing.assert_array_equal(o_sh.cpu().numpy(), obs_c)
        np.testing.assert_array_equal(sh.get_pool(case.M), pool)
        np.testing.assert_array_equal(sh.get_state()['objs'], objs_c)
    finally:
        full.close()
        sh.close()
