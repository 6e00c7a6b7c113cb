"""CPU: batch.constraint_arrays, the one place that turns a constraint setting into one entry per component."""
import numpy as np
import pytest

from scarlet_amd.batch import constraint_arrays, is_scalar_setting

S, K = 3, 4


def test_scalars_fill_the_array():
    for kind in ("symmetric", "monotonic"):
        for v in (True, False, 1, 0, np.bool_(True)):
            a = constraint_arrays(v, S, K, kind)
            assert a.dtype == np.uint8 and a.shape == (S, K) and (a == int(bool(v))).all()
    for kind in ("l0_thresh", "l1_thresh"):
        a = constraint_arrays(0.25, S, K, kind)
        assert a.dtype == np.float32 and a.shape == (S, K) and (a == np.float32(0.25)).all()
        assert (constraint_arrays(0, S, K, kind) == 0).all()            # a threshold of 0 is on (cuts nothing)
    assert is_scalar_setting(None) and is_scalar_setting(True) and is_scalar_setting(0.5) and is_scalar_setting(np.float32(1))
    assert not is_scalar_setting([1, 0]) and not is_scalar_setting(np.zeros((2, 2))) and not is_scalar_setting([[1], [0, 1]])


def test_one_row_for_all_scenes():
    a = constraint_arrays([1, 0, True, False], S, K, "symmetric")
    assert a.tolist() == [[1, 0, 1, 0]] * S
    a = constraint_arrays(np.array([0.5, -1, 0, 2]), S, K, "l1_thresh")
    assert a.tolist() == [[0.5, -1, 0, 2]] * S
    # S == K: a vector is one entry per component
    assert constraint_arrays([1, 0, 0], 3, 3, "monotonic").tolist() == [[1, 0, 0]] * 3


def test_full_array():
    v = np.arange(S * K).reshape(S, K) % 3 == 0
    a = constraint_arrays(v, S, K, "monotonic")
    assert a.dtype == np.uint8 and a.tolist() == v.astype(int).tolist()
    t = np.linspace(-1, 1, S * K).reshape(S, K)
    a = constraint_arrays(t, S, K, "l0_thresh")
    assert np.array_equal(a, np.where(t < 0, -1, t).astype(np.float32))
    assert constraint_arrays(v.tolist(), S, K, "symmetric").tolist() == v.astype(int).tolist()


def test_ragged_lists_are_padded_like_centres():
    a = constraint_arrays([[1, 0], [0, 1, 1, 0], [1, 1, 1]], S, K, "symmetric")
    assert a.tolist() == [[1, 0, 0, 0], [0, 1, 1, 0], [1, 1, 1, 0]]
    a = constraint_arrays([[0.5, None], [None, 1, -2, 0], [0.25]], S, K, "l0_thresh")
    assert a.tolist() == [[0.5, -1, -1, -1], [-1, 1, -1, 0], [0.25, -1, -1, -1]]


def test_none_and_negative_thresholds_mean_off():
    for kind in ("l0_thresh", "l1_thresh"):
        assert (constraint_arrays(None, S, K, kind) == -1).all()
        assert (constraint_arrays(-0.5, S, K, kind) == -1).all()
        assert constraint_arrays([None, -3.0, 0.0, 1e-3], S, K, kind)[1].tolist() == [-1, -1, 0, np.float32(1e-3)]
    with pytest.raises(ValueError):
        constraint_arrays(float("nan"), S, K, "l0_thresh")
    with pytest.raises(ValueError):
        constraint_arrays(None, S, K, "symmetric")                       # a switch is on or off


@pytest.mark.parametrize("bad", [
    [1, 0, 1],                                  # (K - 1,)
    [1, 0, 1, 0, 1],                            # (K + 1,)
    np.ones((S + 1, K)),                        # one scene too many
    np.ones((S, K + 1)),                        # a row longer than K
    np.ones((S, K, 1)),                         # three dimensions
    [[1, 0], [1]],                              # per-scene lists, one scene short
    [[1, 0], [1], [1, 1, 1, 1, 1]],             # a per-scene list longer than K
    [[1, 0], 1, [1]],                           # rows and single entries mixed
])
def test_bad_shapes_raise(bad):
    for kind in ("symmetric", "l1_thresh"):
        with pytest.raises(ValueError):
            constraint_arrays(bad, S, K, kind)
    with pytest.raises(ValueError):
        constraint_arrays(1, S, K, "positive")                           # an unknown setting


def test_layers_of_one_source_must_agree_on_the_switches():
    group = [[0, 0, -1, -1], [-1, 1, 1, 1], [-1, -1, -1, -1]]
    ok = [[1, 1, 0, 1], [0, 1, 1, 1], [1, 0, 1, 0]]
    for kind in ("symmetric", "monotonic"):
        assert constraint_arrays(ok, S, K, kind, group=group).tolist() == ok
        with pytest.raises(ValueError, match="group 0"):
            constraint_arrays([[1, 0, 0, 1], [0, 1, 1, 1], [1, 0, 1, 0]], S, K, kind, group=group)
        with pytest.raises(ValueError, match="group 1"):
            constraint_arrays([[1, 1, 0, 1], [0, 1, 1, 0], [1, 0, 1, 0]], S, K, kind, group=group)
        with pytest.raises(ValueError):
            constraint_arrays([1, 0, 0, 0], S, K, kind, group=group)      # one row for all scenes: scene 0's layers differ
    # thresholds may differ between the layers
    t = constraint_arrays([[0.1, 0.2, -1, -1]] * S, S, K, "l0_thresh", group=group)
    assert t[0, 0] != t[0, 1]
