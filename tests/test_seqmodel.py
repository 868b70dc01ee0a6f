"""The call-sequence harness of tests/seqmodel.py on the CPU: the sequences that tests/test_gpu_sequences.py runs against
Engine, here against CheckerSubject -- the checker behind Engine's interface.

  * every committed (config, seed) passes: the model's counters, books and `_obs` tracking and the legality rules are
    consistent with an eager implementation of Engine's documented behaviour;
  * every planted mistake (seqmodel.BUGS) is caught by at least one committed seed of every config: the sequences do
    reach the orders of calls in which deferred state can be lost, kept too long or shared;
  * the coverage the issue asks for holds, computed from the generator alone."""
import numpy as np
import pytest

import seqmodel as sm


# The planted mistakes run with a quarter of the layout candidates: a reset() of the checker costs 0.2 s at 20000, the
# sequences hold a dozen, and what these tests are about -- which order of calls shows which mistake -- does not depend
# on the size of the pool (5000 candidates leave about 90 valid layouts, more than the 67 envs).
PLANTED_CANDIDATES = 5000


def _run(name, seed, bug=None):
    r = sm.Runner.make(name, "checker", bug=bug, n_candidates=PLANTED_CANDIDATES if bug else sm.N_CANDIDATES)
    r.run(sm.generate(name, seed))
    return r


@pytest.mark.parametrize("name,seed", sm.CASES, ids=[f"{n}-seed{s}" for n, s in sm.CASES])
def test_checker_subject_is_clean(name, seed):
    r = _run(name, seed)
    assert r.n_done > 0                       # every sequence re-initialises rows
    assert r.O.layout_size > r.N


@pytest.mark.parametrize("name", list(sm.CONFIGS))
@pytest.mark.parametrize("bug", list(sm.BUGS))
def test_planted_mistake_is_caught(bug, name):
    caught = []
    for seed in sm.CONFIGS[name]["seeds"]:
        try:
            _run(name, seed, bug)
        except AssertionError as e:
            msg = str(e)
            assert "diverged from the checker" in msg or "after the last op" in msg
            assert "--- reproducer ---" in msg and f"Runner.make({name!r}" in msg
            caught.append((seed, msg.splitlines()[0]))
            break
    print(f"{bug} on {name}: {caught}")
    assert caught, f"no committed seed of {name} notices: {sm.BUGS[bug]}"


@pytest.mark.parametrize("name", list(sm.CONFIGS))
def test_coverage(name):
    pairs, behind_reset, lengths, (hits, misses, off) = sm.coverage(name)
    for ctx in sm.CONTEXTS:
        missing = [k for k in sm.STATE_KINDS if (ctx, k) not in pairs]
        assert not missing, f"{name}: no {missing} directly after / under '{ctx}'"
    assert behind_reset >= 1                  # an expand_tape separated from its rollout_tape by a reset()
    assert hits >= 1 and misses >= 1 and off >= 1
    assert all(sm.LENGTH <= n <= sm.LENGTH + 35 for n in lengths), lengths
    print(f"{name}: ops {lengths}, expansions behind a reset {behind_reset}, prefetch hits / misses / off {hits} / {misses} / "
          f"{off}, (context, kind) pairs " + ", ".join(f"{c}: {sum(v for (cc, _), v in pairs.items() if cc == c)}" for c in sm.CONTEXTS))


def test_the_generator_is_a_pure_function_of_config_and_seed():
    for name, seed in sm.CASES[::4]:
        assert sm.generate(name, seed) == sm.generate(name, seed)
    assert sm.generate("point64-n5", 0) != sm.generate("point64-n5", 1)
    assert sm.generate("point64-n5", 0) != sm.generate("point64-n67", 0)


def test_only_legal_ops_are_emitted_and_illegal_ones_are_refused():
    for name, seed in sm.CASES:
        g = sm.GenState()
        for op in sm.generate(name, seed):
            assert sm.illegal(g, op) is None, (name, seed, op)
            g.apply(op)
    g = sm.GenState()
    assert "before gx_reset" in sm.illegal(g, ("step", dict(aseed=0)))
    g.apply(("reset", dict(check=True)))
    assert "nothing to report" not in (sm.illegal(g, ("check_layouts", {})) or "")
    g.apply(("check_layouts", {}))
    assert "since the last" in sm.illegal(g, ("check_layouts", {}))
    g.apply(("rollout_tape", dict(aseed=0, T=2)))
    assert "reset_done() before reset()" in sm.illegal(g, ("reset_done", {}))
    assert "before reset()" in sm.illegal(g, ("rollout_usl", dict(T=1, obs0=None, correct=False, episode=False)))
    assert sm.illegal(g, ("rollout_usl", dict(T=1, obs0=5, correct=False, episode=False))) is None
    g.apply(("reset", dict(check=False)))
    assert "before the second reset()" in sm.illegal(g, ("reset", dict(check=True)))
    g.apply(("expand_tape", {}))
    assert sm.illegal(g, ("reset", dict(check=True))) is None
    # the adapter refuses what Engine refuses
    r = sm.Runner.make("point64-n5", "checker")
    r.reset(check=True)
    r.rollout_tape(aseed=1, T=2)
    with pytest.raises(RuntimeError, match="before reset"):
        r.S.reset_done()
    with pytest.raises(RuntimeError, match="before reset"):
        r.S.rollout_policy(r.nets.params, 1)


def test_a_failure_names_the_op_and_prints_a_runnable_sequence():
    name, bug = "point64-n5", "speculation_committed"
    for seed in sm.CONFIGS[name]["seeds"]:
        ops = sm.generate(name, seed)
        try:
            sm.Runner.make(name, "checker", bug=bug).run(ops)
        except AssertionError as e:
            msg = str(e)
            break
    else:
        pytest.fail("no seed notices the planted mistake")
    i = int(msg.split(": op ")[1].split()[0])
    assert sm.line(ops[i]) in msg.splitlines()[0]
    body = msg.split("--- reproducer ---\n")[1]
    assert body.splitlines()[-1] == sm.line(ops[i]) and len(body.splitlines()) == i + 3
    # the printed lines run as they are, fail at the last op and not before
    planted = body.replace("'engine'", f"'checker', bug={bug!r}")
    with pytest.raises(AssertionError):
        exec(planted, {})                                             # noqa: S102
    exec("\n".join(planted.splitlines()[:-1]), {})                    # noqa: S102


def test_outputs_are_re_read_at_the_end():
    """the immutability check: an output that changes after it was returned fails finish()"""
    r = sm.Runner.make("point64-n5", "checker")
    r.reset(check=True)
    r.step(aseed=1)
    r.finish()
    r.kept[1][1][0, 0] += np.float32(1)
    with pytest.raises(AssertionError, match="changed after it was returned"):
        r.finish()
