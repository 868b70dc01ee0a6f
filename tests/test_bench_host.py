"""Host-side logic of bench.py that needs no GPU: the round-over-round comparison block and the --dump-outputs writer."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    return bench


def test_previous_round_values_come_from_the_committed_records():
    bench = _bench()
    rnd, prev = bench.previous_round_values()
    recs = sorted(f for f in os.listdir(ROOT) if f.startswith("BENCH_r") and f.endswith(".json"))
    assert recs and rnd == recs[-1][6:9]
    with open(os.path.join(ROOT, recs[-1])) as f:
        rec = json.load(f)
    assert prev["value"] == (float(rec["parsed"]["value"]), recs[-1] + ":parsed.value")
    for k, (v, src) in prev.items():
        assert v > 0 and (src.startswith("BENCH_r") or src.startswith("profiles/")), (k, v, src)
    assert any(k.startswith("other_robots.") for k in prev)


def test_vs_previous_round_flags_what_fell_and_only_that():
    bench = _bench()
    rnd, prev = bench.previous_round_values()
    # a line that repeats the previous round's numbers exactly, except one robot 5 % down and the host-bound loop 6 % down
    robots = {k.split(".", 1)[1]: {"env_steps_per_s": v} for k, (v, _) in prev.items() if k.startswith("other_robots.")}
    victim = sorted(robots)[0]
    robots[victim]["env_steps_per_s"] *= 0.95
    robots["process"] = "fresh child process of bench.py"          # (a string entry rides in the dict)
    line = {"value": prev["value"][0], "other_robots": robots, "preconditioned": {"value": prev["value"][0] * 1.001}}
    if "api_step_loop" in prev:
        line["api_step_loop_env_steps_per_s"] = {"value": prev["api_step_loop"][0] * 0.94}
    out = bench.vs_previous_round(line)
    assert out["previous"] == rnd
    assert out["regressions"] == ["other_robots." + victim]         # the api loop's bar is -10 %: host-bound
    row = out["values"]["other_robots." + victim]
    assert abs(row["change"] + 0.05) < 1e-3 and row["previous"] > row["now"]
    if "api_step_loop" in prev:
        assert out["values"]["api_step_loop"]["threshold"] == bench.HOST_BOUND_THRESHOLD
    if rnd <= "r04":   # rounds 2-4 reported the preconditioned repetition as `value`: compared like for like
        assert out["values"]["value"].get("like_for_like") is False and "preconditioned" in out["values"]


def test_comparable_values_ignore_what_is_not_a_rate():
    bench = _bench()
    vals = bench._comparable_values({"value": 1.0, "other_robots": {"a": {"env_steps_per_s": 2.0}, "process": "x", "b": {"error": "y"}},
                                     "closed_loop_policy_env_steps_per_s": {"error": "z"},
                                     "closed_loop_policy_wider_env_steps_per_s": {"hidden_128": 3.0, "hidden_256": "err"}})
    assert vals == {"value": 1.0, "other_robots.a": 2.0, "closed_loop_policy.hidden_128": 3.0}


def test_dump_outputs_writes_the_last_epoch_within_the_byte_limit(tmp_path, monkeypatch):
    import numpy as np
    import torch
    bench = _bench()
    T, N, D, A = 3, 50, 4, 2
    g = torch.Generator().manual_seed(1)
    obs, rew, cost, done = (torch.rand(T, N, D, generator=g),) + tuple(torch.rand(T, N, generator=g) for _ in range(3))
    # rollout()'s four tensors, small enough to go out whole
    info = bench.dump_outputs(str(tmp_path / "whole"), (obs, rew, cost, done), D, A)
    assert info["env_columns"] == N and info["env_sample_seed"] is None
    for name, t in zip(("obs", "reward", "cost", "done"), (obs, rew, cost, done)):
        a = np.load(tmp_path / "whole" / f"{name}.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, t.numpy())
    # the gathered packed rows (world, T, N, D + A + 3) of a hand-off, over the limit: the same env columns everywhere
    act = torch.rand(T, N, A, generator=g)
    packed = torch.cat([obs, act, rew[..., None], cost[..., None], done[..., None]], -1)[None]
    monkeypatch.setattr(bench, "DUMP_BYTES", packed.numel() * 4 // 2)
    runs = []
    for k in range(2):
        info = bench.dump_outputs(str(tmp_path / f"s{k}"), packed, D, A)
        assert 0 < info["env_columns"] < N and info["arrays"] == ["action", "cost", "done", "obs", "reward"]
        runs.append({n: np.load(tmp_path / f"s{k}" / f"{n}.npy") for n in info["arrays"]})
        assert sum(a.nbytes for a in runs[-1].values()) <= bench.DUMP_BYTES
    cols = [int(np.argmax((rew[0].numpy() == v))) for v in runs[0]["reward"][0, 0]]
    assert cols == sorted(cols) and len(set(cols)) == len(cols)
    np.testing.assert_array_equal(runs[0]["obs"][0], obs[:, cols].numpy())
    np.testing.assert_array_equal(runs[0]["action"][0], act[:, cols].numpy())
    np.testing.assert_array_equal(runs[0]["done"][0], done[:, cols].numpy())
    for n in runs[0]:
        np.testing.assert_array_equal(runs[0][n], runs[1][n])
