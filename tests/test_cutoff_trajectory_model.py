"""CPU model of the HIP cutoff's lookup-free, block-parallel bisection (effort_amd/csrc/cutoff_device.h, "THE BISECTION WITHOUT ITS
LOOKUPS") against the oracle's findCutoff32.  The device code replaces every use of a count inside the reference's loop --
the steering comparison and the two count-driven exit tests -- with comparisons of the threshold's bf16 CELL against five
order statistics of the values; this restates that control flow in numpy f32 arithmetic -- including the hand-over to the
closed-form tail and the ballot rounds for value ranges wider than the table -- asserts every shortcut against the count
it stands for, and compares the float BITS with the C oracle over seeded inputs that leave the loop through every exit.  The five
order statistics are also found the way the device finds them since round 5 -- from the HISTOGRAM of the cells, one wave, two
levels (`_device_order_statistic`), over the cells between the bounds and over the fixed window plain grids count into before the
value range is known -- and must be the same cells.  The model itself lives in tests/cutoff_model.py (it also reports the path it took:
tests/test_cutoff_cases_cpu.py); this file runs it over 40 seeds of six kinds at each of the four table sizes.  (The device code itself is compared with the oracle by the -m gpu tests: test_cutoff_*.)"""
import numpy as np
import pytest

from tests.cutoff_cases import kind_inputs
from tests.cutoff_model import CAPS, model_cutoff


@pytest.mark.parametrize("kind", ["gauss", "heavy", "zeros", "wide", "few", "tiny"])
def test_lookup_free_bisection_model_matches_oracle(oracle_cpu, kind):
    """The model at every table size a workgroup of 128 .. 1024 threads gives (CAPS): every shortcut asserted inside the model against
    the count it stands for, the window's order statistics included, and the cutoff's bits the oracle's."""
    mism = 0
    for seed in range(40):
        v, pr = kind_inputs(seed, kind)
        for effort in (0.0, 0.02, 0.1, 0.25, 0.5, 0.9, 1.0):
            want, _ = oracle_cpu.find_cutoff(v, pr, 0, effort)
            for cap in CAPS:
                got, _ = model_cutoff(v, pr, oracle_cpu.effort_to_q(effort), cap=cap)
                if np.float32(want).view(np.uint32) != np.float32(got).view(np.uint32):
                    mism += 1
    assert mism == 0
