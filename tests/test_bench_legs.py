"""CPU: a plain bench.py run does only what its headline line needs; the CPU oracle leg and the other configs'
child runs belong to `--full` (single GPU), and `--no-cpu` / `--no-other` still drop them there."""
import pytest


def _legs(argv, world=1, rank=0):
    import bench
    return bench.extra_legs(bench.parse_args(["--steps", "3", "--warmup", "1"] + argv), world, rank)


def test_plain_run_has_no_extra_legs():
    assert _legs([]) == (False, False)
    for cfg in ("c3", "c5"):
        assert _legs(["--config", cfg]) == (False, False)


def test_full_run_has_both_legs():
    assert _legs(["--full"]) == (True, True)
    assert _legs(["--full", "--no-cpu"]) == (True, False)
    assert _legs(["--full", "--no-other"]) == (False, True)


@pytest.mark.parametrize("argv", [["--config", "c3"], ["--config", "c5"], ["--scenes", "100"], ["--strong"],
                                  ["--no-symmetric"], ["--no-monotonic"]])
def test_other_configs_only_for_the_unmodified_c2_workload(argv):
    assert _legs(["--full"] + argv) == (False, True)


def test_full_adds_nothing_on_several_ranks():
    assert _legs(["--full", "--gpus", "2"], world=2, rank=0) == (False, False)
    assert _legs(["--full", "--gpus", "2"], world=2, rank=1) == (False, False)


def test_other_configs_children_run_full(monkeypatch):
    """the c3 / c5 child runs keep their own CPU legs, as they had before `--full` existed"""
    import subprocess
    import bench
    cmds = []

    def run(cmd, **kw):
        cmds.append(cmd)
        raise subprocess.TimeoutExpired(cmd, 0)
    monkeypatch.setattr(subprocess, "run", run)
    out = bench.run_other_configs(bench.parse_args(["--full", "--steps", "20", "--warmup", "5"]))
    assert sorted(out) == ["c3", "c5"] and [c[c.index("--config") + 1] for c in cmds] == ["c3", "c5"]
    assert all("--full" in c and "--no-cpu" not in c for c in cmds)
