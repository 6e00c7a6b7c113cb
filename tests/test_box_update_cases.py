"""CPU: the cases of tests/box_update_cases.py are what tests/test_gpu_box_update.py takes them for -- every one decided
in the reference alone (float32 and float64 oracle: same support, same centre, 1e-6), none exempt, and the stages the
table expects cover the 63 x 63 box, the 127 x 127 box and the full-frame kernel at every frame."""
import numpy as np
import pytest

import box_update_cases as bc


@pytest.fixture(scope="module", autouse=True)
def oracle_lib():
    from oracle import build as obuild
    obuild.build()


@pytest.mark.parametrize("frame", [f[0] for f in bc.FRAMES])
def test_every_case_is_decided(frame):
    for phase, scenes in bc.frame_cases(frame).items():
        for case in (c for sc in scenes for c in sc):
            assert bc.decided(case, phase), "%s (%s) is not decided: give it another seed in RESEED" % (case["id"], phase)
            # the stage is the same whichever oracle it is read from
            assert bc.expected_stage(case, phase, np.float32) == bc.expected_stage(case, phase, np.float64), case["id"]


@pytest.mark.parametrize("frame", [f[0] for f in bc.FRAMES])
def test_the_expected_stages_cover_every_hand_off(frame):
    """each stage is expected for a component whose sweep decided it, in the constructor phase alone; in a frame that
    holds the whole 127 x 127 box the levels either side of each hand-off are there with the stage the derivation gives"""
    _, H, W, _, _ = bc.FRAME[frame]
    got = {}
    for case in (c for sc in bc.frame_cases(frame)["ctor"] for c in sc):
        if bc.is_sweep(case, "ctor") and not case["sym"]:
            Lp, cen = bc.sweep_lp(case, "ctor")
            got.setdefault(Lp, set()).add((bc.expected_stage(case, "ctor"), bc.box_lall(H, W, cen, bc.R_LARGE) >= 126))
    assert {st for v in got.values() for st, _ in v} == {bc.SMALL, bc.LARGE, bc.FULL}, got
    want = {59: bc.SMALL, 60: bc.LARGE, 62: bc.LARGE, 63: bc.LARGE, 123: bc.LARGE, 124: bc.FULL, 126: bc.FULL, 127: bc.FULL}
    for Lp, st in want.items():
        assert Lp in got, "no case with Lp = %d at %s" % (Lp, frame)
        for stage, whole_box in got[Lp]:
            assert stage == st or not whole_box, (frame, Lp, stage)
        assert any(stage == st for stage, _ in got[Lp]), (frame, Lp, got[Lp])
    if frame == "66x24":                  # the short frame: the 127 x 127 box's own last level, 87, ends the sweep
        assert got[84] == {(bc.LARGE, False)} and got[85] == {(bc.FULL, False)} and got[87] == {(bc.FULL, False)}, got


def test_every_frame_selects_its_instance_and_every_switch_is_used():
    """the frames are the ones launch_plan.h gives each instance to, and the switches appear at every frame"""
    for name, H, W, inst, opt in bc.FRAMES:
        streamed = H > 256 or W > 256
        want = "<0,0>" if streamed else "<8,128>" if (H, W, opt) == (128, 128, None) else \
            "<16,256>" if (H, W, opt) == (256, 256, None) else "<8,0>" if H <= 128 and W <= 128 else "<16,0>"
        assert (H > 64 or W > 64) and inst == want, name
        for phase, scenes in bc.frame_cases(name).items():
            cases = [c for sc in scenes for c in sc]
            assert len({c["id"] for c in cases}) == len(cases)
            assert sum(1 for c in cases if not c["mono"]) == 1, (name, phase)
            assert any(c["sym"] and c["mono"] and c["start"] != c["peak"] for c in cases), (name, phase)
            assert {c["rim"] for c in cases if c["mono"] and not c["sym"]} == {0, 1} or phase != "ctor", (name, phase)
            assert not any(c["rim"] for c in cases if c["sym"] or not c["mono"])
            assert any(c["l0"] >= 0 for c in cases) or phase == "it0", (name, phase)
            assert any(c["l1"] >= 0 for c in cases) or phase == "it4", (name, phase)
            for c in cases:                              # max_pixel's 5 x 5 window about the start lies inside the frame
                assert 2 <= c["start"][0] < H - 2 and 2 <= c["start"][1] < W - 2, c["id"]
                assert max(abs(c["start"][0] - c["peak"][0]), abs(c["start"][1] - c["peak"][1])) <= 2, c["id"]
    # the soft flip about the array middle: expected on the full-frame kernel, the exact middle of the odd frame included
    for name in ("72x80", "73x81"):
        case = bc.frame_cases(name)["it0"][0][1]
        _, H, W, _, _ = bc.FRAME[name]
        assert case["sym"] and case["peak"] == (H // 2, W // 2) and bc.expected_stage(case, "it0") == bc.FULL
        assert bc.sweep_lp(case, "it0")[0] <= 59                 # ... which the sweep alone would have left to the small box
