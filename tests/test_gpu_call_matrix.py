"""GPU half of the calling-condition matrix (tests/call_cells.py): every (variant, subject) cell that is not listed in EXCLUSIONS.

A cell runs the subject under the condition and compares it, by the one class rule of `call_cells.klass`, with the same subject under
the canonical call -- bit equality for y, dx and every deterministic gradient -- or asserts the refusal.  The canonical call of every
subject is the one an existing matrix judges against fp64 (tests/test_call_matrix.py holds the subjects to their rows); it is computed
once per subject and shared.  DESIGN.md section 4e lists the subjects, the conditions, the exclusions and what the matrix found."""
import pytest

from call_cells import VARIANT, cells, live_of

pytestmark = pytest.mark.gpu

CELLS = cells(gpu=True)


@pytest.mark.parametrize("variant,sid", CELLS, ids=[f"{v}-{s}" for v, s in CELLS])
def test_call_cell(variant, sid, gpu_lib):
    try:
        VARIANT[variant][1](live_of(sid))
    except Exception as e:
        if any(w in str(e) for w in ("illegal memory access", "HIP error", "hipError")):      # a device fault: nothing more may run on this device
            pytest.exit(f"{variant}-{sid}: device fault, the run ends here: {e}", returncode=3)
        raise
