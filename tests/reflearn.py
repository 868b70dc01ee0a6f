"""reflearn.py -- TEST INFRASTRUCTURE ONLY: the reference learners' own code on the CPU, loaded live from a checkout of
the reference ($GUARDX_REFERENCE, default /root/reference: the convention of tests/golden/gen_reference_golden.py), for
tests/test_reference_learners.py.  Nothing of the checkout is copied: what is needed is read from its files when a test
asks for it, and a test skips where the checkout is absent (available()).

  core(learner, one_episode)    safe_rl_libX/<learner>[_one_episode]/<learner>_core.py imported by path.  Beyond numpy,
                                scipy and torch these modules import gym.spaces (Box, Discrete) and, for LPG, qpsolvers:
                                where those do not import, empty stand-ins are in sys.modules for the duration of the
                                import and are removed again, whatever happens.  jax and mujoco are never stubbed
                                (tests/test_pin_machinery.py decides by whether they import).
  main(learner, names, ...)     the learners' main files import jax, MPI and the env at module level, so they are never
                                imported: the file is parsed and only the named top-level classes / functions (the
                                *BufferX classes, cg, auto_grad, auto_hession_x) are compiled, into a namespace that
                                supplies np, torch, scipy, core, device = cpu, EPS and mpi_statistics_scalar.
  mpi_statistics_scalar         taken from utils/mpi_tools.py the same way, over one-process stand-ins for the MPI
                                helpers it calls (a sum over one process is the float32 value it was given).
  same_code(learner, name)      whether a class or function of the plain core and of its *_one_episode twin are the same
                                code (their syntax trees compared, so comments and blank lines do not count).
"""
import ast
import functools
import importlib.util
import os
import sys
import types

import numpy as np

REFERENCE = os.environ.get("GUARDX_REFERENCE", "/root/reference")
LIBX = os.path.join(REFERENCE, "safe_rl_libX")
STAND_INS = ("gym", "gym.spaces", "qpsolvers")


def available():
    return os.path.isdir(LIBX)


def _dir(learner, one_episode=False):
    return os.path.join(LIBX, learner + ("_one_episode" if one_episode else ""))


def _stand_in(name):
    m = types.ModuleType(name)
    if name == "gym.spaces":
        class Box:
            def __init__(self, shape):
                self.shape = tuple(shape)

        class Discrete:
            def __init__(self, n):
                self.n = n
        m.Box, m.Discrete = Box, Discrete
    if name == "qpsolvers":
        m.solve_qp = None            # (imported by name in lpg_core.py, called nowhere on the paths compared here)
    return m


def _importable(name):
    if name in sys.modules:
        return True
    try:
        return importlib.util.find_spec(name) is not None
    except (ImportError, ValueError):
        return False


@functools.lru_cache(maxsize=None)
def core(learner, one_episode=False):
    """the reference's <learner>_core module (never entered into sys.modules)"""
    path = os.path.join(_dir(learner, one_episode), learner + "_core.py")
    placed = []
    try:
        for name in STAND_INS:
            if not _importable(name):
                sys.modules[name] = _stand_in(name)
                placed.append(name)
        if "gym" in placed:
            sys.modules["gym"].spaces = sys.modules["gym.spaces"]
        spec = importlib.util.spec_from_file_location("reflearn_%s%s_core" % (learner, "_one_episode" if one_episode else ""), path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for name in placed:
            sys.modules.pop(name, None)


def _nodes(path, names):
    import warnings
    with open(path) as f, warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (escape sequences in docstrings of code that is not compiled here)
        tree = ast.parse(f.read(), filename=path)
    found = {n.name: n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names}
    missing = [n for n in names if n not in found]
    if missing:
        raise LookupError(f"{path}: no top-level {missing}")
    return [found[n] for n in names]


def _compile_into(path, names, namespace):
    import warnings
    module = ast.Module(body=_nodes(path, names), type_ignores=[])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exec(compile(module, path, "exec"), namespace)
    return [namespace[n] for n in names]


def same_code(learner, name, file="core"):
    """the plain learner's and its *_one_episode twin's `name` (a top-level class or function of <learner>_core.py, or of
    <learner>.py with file='main') are the same code"""
    fn = learner + ("_core.py" if file == "core" else ".py")
    a, b = (_nodes(os.path.join(_dir(learner, e), fn), [name])[0] for e in (False, True))
    return ast.dump(a) == ast.dump(b)


def _one_process_sum(x):
    """utils/mpi_tools.py:mpi_sum for one process: what an Allreduce(SUM) into a float32 buffer over one rank leaves"""
    scalar = np.isscalar(x)
    buf = np.asarray([x] if scalar else x, dtype=np.float32).copy()
    return buf[0] if scalar else buf


@functools.lru_cache(maxsize=None)
def mpi_statistics_scalar():
    for d in (os.path.join(LIBX, "utils"), os.path.join(LIBX, "guard_utils"), os.path.join(REFERENCE, "safe_rl_lib", "utils")):
        path = os.path.join(d, "mpi_tools.py")
        if os.path.isfile(path):
            break
    else:
        raise LookupError("no utils/mpi_tools.py in the reference checkout")
    ns = dict(np=np, mpi_sum=_one_process_sum)
    return _compile_into(path, ["mpi_statistics_scalar"], ns)[0]


def main(learner, names, one_episode=False):
    """the named top-level classes / functions of safe_rl_libX/<learner>[_one_episode]/<learner>.py, in the order asked"""
    import scipy
    import scipy.signal  # noqa: F401
    import torch
    ns = dict(np=np, torch=torch, scipy=scipy, core=core(learner, one_episode), device=torch.device("cpu"), EPS=1e-8,
              mpi_statistics_scalar=mpi_statistics_scalar())
    return _compile_into(os.path.join(_dir(learner, one_episode), learner + ".py"), list(names), ns)


def actor_critic(learner, D, A, hidden, seed, one_episode=False):
    """the reference's MLPActorCritic(observation_space of D entries, Box action space of A, hidden_sizes=(hidden, hidden))
    on the CPU, float32, torch's default initialisation under `seed`"""
    import torch
    c = core(learner, one_episode)
    was = torch.cuda.is_available
    torch.cuda.is_available = lambda: False          # the class picks its own device: keep it off any GPU
    try:
        torch.manual_seed(seed)
        return c.MLPActorCritic(c.Box((D,)), c.Box((A,)), hidden_sizes=(hidden, hidden))
    finally:
        torch.cuda.is_available = was


def c_critic(learner, D, A, hidden, seed, one_episode=False):
    """the reference's C_Critic(D, A, (hidden, hidden), Tanh, cpu), float32, torch's default initialisation under `seed`"""
    import torch
    torch.manual_seed(seed)
    return core(learner, one_episode).C_Critic(D, A, (hidden, hidden), torch.nn.Tanh, torch.device("cpu"))
