"""Engine as a state machine: the random call sequences of tests/seqmodel.py against Engine, with the CPU checker as the
model.  Every legal sequence of public calls must give the checker's bits whatever the engine has deferred between the
calls (a requested or a speculated reset_done, the layout-size minimum, the pool prefetch, tape tokens, the noise
counters, the Python-side books) -- tests/seqmodel.py lists the ops, the legality rules and what is compared.

One engine per sequence, closed at the end.  Nothing is retried or shrunk here: a mismatch is reported once, with the seed,
the index of the failing op and the sequence up to it as runnable Python.  The same sequences run against the checker's own
adapter, and against planted mistakes, in tests/test_seqmodel.py (no GPU)."""
import time

import pytest

import seqmodel as sm

pytestmark = pytest.mark.gpu


def _run(name, ops):
    import torch
    t0 = time.perf_counter()
    r = sm.Runner.make(name, "engine")
    try:
        r.run(ops)
        torch.cuda.synchronize()
        stats = r.S.prefetch_stats()
    finally:
        r.close()
    return r, stats, time.perf_counter() - t0


@pytest.mark.parametrize("name,seed", sm.CASES, ids=[f"{n}-seed{s}" for n, s in sm.CASES])
def test_sequence_equals_the_checker(name, seed):
    ops = sm.generate(name, seed)
    r, (hits, misses, _), dt = _run(name, ops)
    print(f"{name} seed {seed}: {len(ops)} ops, {r.n_done} done rows, {len(r.kept)} outputs re-read at the end, "
          f"prefetch hits / misses {hits} / {misses}, {dt:.2f} s")
    assert r.n_done > 0
    g = sm.final_state(ops)
    assert (hits, misses) == (g.hits, g.misses), "prefetched pools used / discarded, against the generator's count"


# ---------------------------------------------------------------------------------------------------------------------
# findings of the random sequences, each as its shortest reproducing sequence
# ---------------------------------------------------------------------------------------------------------------------
def test_reset_done_after_a_packed_rollout():
    """Found by point128-n67 seed 1 (op 55).  After rollout(packed=True) Engine._obs is a view of the packed rows (row
    stride D + A + 3); reset_done() handed its address to gx_reset_done, which reads dense (N, D) rows: every row but the
    first of the returned observation came from the wrong place.  reset_done() now passes a dense copy of such a view."""
    ops = [("reset", dict(check=True)), ("rollout", dict(aseed=1, T=3, packed=True)), ("reset_done", {}),
           ("set_path", dict(mode=1)), ("rollout", dict(aseed=2, T=2, packed=True)), ("reset_done", {}), ("reset_done", {})]
    _run("point64-n67", ops)


def test_reset_done_repeated_behind_get_state():
    """Found by point64-n67 seed 2.  step(); reset_done() leaves the re-initialisation requested; get_state() installs it
    (it is part of the state) -- and a reset_done() repeated after that raised "gx_reset_done_commit: the last hot-path
    call was not a speculating gx_step_rd", although reset_done() twice in a row is legal and idempotent.  get_state() now
    notes for which speculated observation it installed the request, and reset_done() hands that one out again."""
    ops = [("reset", dict(check=True)), ("set_state", dict(sseed=7, fields="all")), ("step", dict(aseed=1)), ("reset_done", {}),
           ("get_state", {}), ("reset_done", {}), ("get_state", {}), ("step", dict(aseed=2)), ("get_state", {}),
           ("reset_done", {}), ("reset_done", {}), ("step", dict(aseed=3)), ("get_state", {})]
    _run("point64-n67", ops)
    _run("ant64-n5", ops)
