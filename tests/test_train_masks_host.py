"""The mask-matched float64 oracle (oracle/scream_ref.py: masks / record_masks / sign; tests/train_ref.py) on the CPU, with the
fp32 CPU oracle standing in for the path under test.  Runs everywhere; the GPU's gradients take the same rule in
tests/test_gpu_train*.py."""
import pytest
import torch

import train_ref as T
from scream_amd.synthetic import make_state_dict


def _old_rule(g, g64, g32):
    """What the model-gradient tests asserted before: against float64 under ITS OWN masks, max(4 x the fp32 oracle's error,
    5e-4) -- the fp32 oracle's error including its mask flips."""
    return [k for k in g64 if not T.rel(g[k], g64[k]) <= max(4 * T.rel(g32[k], g64[k]), 5e-4)]


@pytest.mark.parametrize("ns,nc,n,m", [(1, 1, 700, 900), (2, 2, 690, 910)])
def test_fp32_oracle_meets_the_rule_under_its_own_masks_and_wrong_gradients_do_not(ns, nc, n, m):
    """The seeds and sizes of test_gpu_train.py::test_model_gradients_against_float64.

    1. The hook is exact: a run that is GIVEN the masks it would have computed (relu(x) -> x * m, abs(x) -> x * s) returns the
       gradients of the plain run bit for bit, in fp32 and in float64.
    2. The fp32 oracle's gradients meet the rule of train_ref.rule against float64 under the fp32 run's masks, and every
       tensor stays under the floor of 5e-6 -- where float64 under its own masks leaves the (1,1) model's
       stem.0.v_proj.weight at 5.5e-4 (one hidden unit of stem.0 within rounding of zero).
    3. Negative controls, each a gradient set that is WRONG and that the former bar max(4 x e32, 5e-4) against float64 under
       its own masks passes (asserted here, so the statement stays true): (a) one deep tensor times 1 + 1e-4; (b) one row of
       one weight gradient zeroed, the row that holds 1e-4 .. 4e-4 of the tensor's norm (a weight row fed by a mostly
       inactive unit; about what one padded row leaking into a sum over a few thousand rows moves).  The rule reports
       both, and exactly the tampered tensor."""
    torch.manual_seed(0)
    sd = make_state_dict(5 + ns, 256, ns, nc)
    pair = T.make_pair(ns, n, m)
    own32, own64 = {}, {}
    _, g32 = T.oracle_grads(sd, *pair, torch.float32, record=own32)
    _, g64 = T.oracle_grads(sd, *pair, torch.float64, record=own64)
    assert len(own32) == len(own64) == (2 * ns + 2 * nc) + 2 + 1  # block applications, coor_mlp's two relus, the L1 sign
    # 1. the hook is exact
    _, g32m = T.oracle_grads(sd, *pair, torch.float32, masks=own32)
    _, g64own = T.oracle_grads(sd, *pair, torch.float64, masks=own64)
    for k in sd:
        assert torch.equal(g32m[k], g32[k]), k
        assert torch.equal(g64own[k], g64[k]), k
    # 2. the rule, under the masks of the path under test
    _, g64m = T.oracle_grads(sd, *pair, torch.float64, masks=own32)
    assert not T.rule("fp32 oracle (%d,%d) under its own masks" % (ns, nc), g32, g64m, g32m)
    e_mask = {k: T.rel(g32[k], g64m[k]) for k in sd}
    e_plain = {k: T.rel(g32[k], g64[k]) for k in sd}
    print("worst against float64 under its own masks %.3g, under the fp32 run's masks %.3g; the two float64 oracles differ by %.3g"
          % (max(e_plain.values()), max(e_mask.values()), max(T.rel(g64m[k], g64[k]) for k in sd)))
    assert max(e_mask.values()) <= T.FLOOR, max(e_mask, key=e_mask.get)
    # 3a. a deep tensor off by 1e-4
    deep = "stem.0.merge.weight"
    wrong = dict(g32)
    wrong[deep] = g32[deep] * (1 + 1e-4)
    assert not _old_rule(wrong, g64, g32)
    assert [b[0] for b in T.rule("negative control: %s x (1 + 1e-4)" % deep, wrong, g64m, g32m)] == [deep]
    # 3b. one row of a weight gradient lost
    name = "cross.0.mlp.0.weight"
    share = torch.linalg.norm(g32[name].double(), dim=1) / torch.linalg.norm(g32[name].double())
    rows = torch.nonzero((share >= 1e-4) & (share <= 4e-4)).flatten()
    assert len(rows) > 0, "no row of %s holds 1e-4 .. 4e-4 of its norm" % name
    row = int(rows[torch.argmax(share[rows])])
    wrong = dict(g32)
    wrong[name] = g32[name].clone()
    wrong[name][row] = 0
    assert not _old_rule(wrong, g64, g32)
    assert [b[0] for b in T.rule("negative control: row %d of %s zeroed (%.3g of its norm)" % (row, name, float(share[row])),
                                 wrong, g64m, g32m)] == [name]
