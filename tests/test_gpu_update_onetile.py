"""The one-tile update kernel (apply_rows_kernel with its gradient rows in dense groups) leaves every bit where it was.

The fixtures, tests/golden/onetile_update_bits.json, are SHA-256 of the float32 table and losses of five steps at
B = 4096, d = 200, recorded on MI355X with the library of the commit BEFORE the dense groups
(tools/dev/onetile_bits.py with GE_LIB naming that library).  The workloads are tests/onetile_cases.py's.

Groups with DEAD slots (a listed slot whose pair is not hinge-active) are what the dense walk changes, so the cases
that have them assert it from the losses: between 20 % and 80 % of the pairs live in every hashed step.  Those are
margin 0.2 in deterministic mode, after 600 deterministic warm-up steps (a fresh table leaves every pair live at that
margin), and margin 0.0 in default mode without hot rows (that workload cannot be trained to margin 0.2 without rows
of more than 16 slots appearing; at margin 0.2 its pairs are all live and the case checks full groups, as margin 5.0
does).  At margin 5.0 every pair is live and every item size from 2 to 16 appears.  Every case reproduced itself run to
run when the fixtures were recorded (no case was dropped); a null fixture would mean one did not, and fails."""
import json
import os

import numpy as np
import pytest

import onetile_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bits(golden_dir):
    with open(os.path.join(golden_dir, "onetile_update_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("margin", C.MARGINS)
@pytest.mark.parametrize("model", C.MODELS)
def test_deterministic_steps_keep_their_bits(bits, model, margin):
    """Trainer(deterministic=True), FB15k-shaped: ~120 hot rows a step, their items parked and reduced in item order."""
    want = bits[C.det_key(model, margin)]
    assert want is not None
    got, live = C.run_det(model, margin)
    print(model, margin, got, "live", live)
    if margin >= 1.0:
        assert all(v == 1.0 for v in live), live
    else:
        assert all(0.2 <= v <= 0.8 for v in live), live
    assert got == want


@pytest.mark.parametrize("margin", C.PLAIN_MARGINS)
@pytest.mark.parametrize("model", C.MODELS)
def test_default_mode_without_hot_rows_keeps_its_bits(bits, model, margin):
    """Default mode on a workload in which no row has more than 16 slots (no float atomics, so the step is reproducible):
    relation rows of 2 ... 16 slots by construction, checked here from the ids of every step."""
    want = bits[C.plain_key(model, margin)]
    assert want is not None
    got, counts, live = C.run_plain(model, margin)
    for c in counts:
        assert c.max() <= C.ITEM_CAP
        for lo, hi in ((2, 4), (5, 8), (9, 12), (13, 16)):
            assert np.count_nonzero((c >= lo) & (c <= hi)) > 0, (lo, hi)
    print(model, margin, got, "live", live)
    if margin >= 1.0:
        assert all(v == 1.0 for v in live), live
    elif margin == 0.0:
        assert all(0.2 <= v <= 0.8 for v in live), live
    assert got == want
