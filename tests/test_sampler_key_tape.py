"""The layout sampler's key tape (gx_kernels.hip, sample_phase1_kernel / sample_phase2_kernel): with the reference's 8
hazards, phase 1 keeps the 80 hazard try keys of the `rng, rng1 = split(rng)` chain in registers and stores those of its
survivors by phase-1 slot; phase 2 reads them instead of walking the chain again.  The tape holds GX_SAMPLE_TAPE_CAP
slots (read at engine creation); a wave whose survivors do not all have an entry walks the chain as before.  Whatever
the capacity, object count or form, the pool -- size, rows, order -- is the CPU checker's."""
import numpy as np
import pytest

from helpers import task_config


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _check_pools(cfg, oracle, n_candidates, resets=2):
    """`resets` consecutive reset()s (the first samples inline, the later ones take the prefetched pool): pool and
    reset observations equal the checker's"""
    from guardx_amd import Engine
    E = Engine(cfg, n_candidates=n_candidates)
    O = oracle.OracleEngine(cfg, n_candidates=n_candidates, env_total=E._cfg.env_total, env_offset=E._cfg.env_offset)
    try:
        for _ in range(resets):
            np.testing.assert_array_equal(E.reset().cpu().numpy(), O.reset())
            assert E.layout_size == O.layout_size > 0
            np.testing.assert_array_equal(E.get_pool(E.layout_size), O.get_pool(O.layout_size))
    finally:
        E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 5, 29])
def test_default_arena_at_a_million_candidates(torch_cuda, oracle, seed):
    """the headline's sampler: 8 hazards, 1e6 candidates, the default tape (every survivor has an entry)"""
    _check_pools(task_config(64, seed=seed, num_steps=20), oracle, 1_000_000)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["0", "1061", "9000"])
def test_tape_capacity_mixes_tape_and_walk(torch_cuda, oracle, monkeypatch, cap):
    """capacity 0 (every wave walks), one that ends inside a wave (slot 1061 = 16 waves + 37 lanes), and one far below
    the ~37 k survivors of 150 k candidates: waves on the tape and waves that walk in one launch.  The grid cap makes
    phase 1 hand out its slots over many grid-stride rounds, so which candidates land below the capacity varies."""
    monkeypatch.setenv("GX_SAMPLE_TAPE_CAP", cap)
    monkeypatch.setenv("GX_SAMPLE_GRID_CAP", "64")
    _check_pools(task_config(96, seed=13, num_steps=20), oracle, 150_000, resets=3)


@pytest.mark.gpu
@pytest.mark.parametrize("hazards,pillars", [(4, 4), (8, 8)])
def test_pillar_arenas_on_the_three_phase_form(torch_cuda, oracle, monkeypatch, hazards, pillars):
    """hazards + pillars = 8: the tape holds the pillars' keys too; 8 + 8: no tape instantiation, today's walk.  Both on
    the three-phase form (forced: the form is otherwise picked by geometry)"""
    monkeypatch.setenv("GX_SAMPLE_FUSED", "0")
    cfg = task_config(96, seed=17, num_steps=20, hazards_num=hazards, pillars_num=pillars, observe_pillars=True,
                      pillars_keepout=0.3, pillars_size=0.2, placements_extents=[-3, -3, 3, 3])
    _check_pools(cfg, oracle, 200_000)


@pytest.mark.gpu
@pytest.mark.parametrize("hazards", [3, 6])
def test_hazard_counts_without_a_tape(torch_cuda, oracle, hazards):
    """object counts with no tape instantiation keep the chain walk in both phases"""
    _check_pools(task_config(64, seed=2, num_steps=20, hazards_num=hazards), oracle, 200_000)
