"""CPU: the numpy loop the gated and the trimmed batch tests are held to (batch_ref.reference_loop), on its own.

The GPU end-to-end tests (test_gpu_batch_gate.py, test_gpu_batch_trim.py) assert these figures on the reference before they look
at the device; here they are checked where there is no device: on the three large clouds of batch_ref.CASES a gate of 0.05 keeps
29 -> 200 -> 200, 16 -> 120 -> 130 -> 130 and 121 -> 1025 -> 1025 points per pass and ends with exactly the non-outliers, a gate
of 0.03 keeps nothing at pass 0, a trim to the closest half keeps 135, 97 and 578 points in every pass, and no decision comes
closer to going the other way than 1e-4 relative -- a flipped mask is never rounding."""
import numpy as np
import pytest

from batch_ref import CASES, gate_case, keep_closest, keep_within, reference_loop

KEPT_GATED = [[29, 200, 200], [16, 120, 130, 130], [121, 1025, 1025]]
KEPT_TRIMMED = [135, 97, 578]


@pytest.mark.parametrize("case", range(3), ids=[str(c) for c in CASES[:3]])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reference_loop_gated_and_trimmed(orc, dtype, case):
    A, M, is_out = gate_case(*CASES[case], dtype=dtype)
    w = reference_loop(orc, A, M, keep_within(0.05), 40, 1e-6)
    want = KEPT_GATED[case]
    print(f"{CASES[case]}: gated at 0.05 keeps {w['kept']}, margin {w['margin']:.3e}, iterations {w['iterations']}")
    k = min(len(w["kept"]), len(want))   # (the reference stops on the pass the device matches once more on: the series may end one short)
    assert k >= 3 and w["kept"][:k] == want[:k] and set(w["kept"][k:]) <= {want[-1]}
    assert w["kept"][0] < w["kept"][-1]     # the kept set changes between passes
    assert np.array_equal(w["mask"], ~is_out)
    assert w["margin"] >= 1e-4
    assert reference_loop(orc, A, M, keep_within(0.03), 40, 1e-6)["kept"] == [0]
    w = reference_loop(orc, A, M, keep_closest(0.5), 40, 1e-6)
    print(f"{CASES[case]}: trimmed to 0.5 keeps {w['kept']}, smallest K-th gap {w['margin']:.3e}, iterations {w['iterations']}")
    assert set(w["kept"]) == {KEPT_TRIMMED[case]}
    assert w["margin"] >= 1e-4
