"""CPU: the batches and decoys of tests/stream_order_cases.py are what tests/test_stream_order_gpu.py needs them to be.

Building a case runs the reference or model on the real batch AND on the decoy (that is the acceptance test: a decoy the oracle
or a model refused would raise there) and checks that every range of the decoy lies inside the real slabs.  Here: the decoy has
the real arrays' names, shapes and dtypes, so that it can be copied over them; and its answer differs from the real one in at
least 90 % of the items of every output -- a condition on the inputs, chosen to hold, not a measurement."""
import numpy as np
import pytest

from tests import stream_order_cases as soc


@pytest.mark.parametrize("name", list(soc.CASES))
def test_decoy_is_valid_and_tells(name):
    c = soc.case(name)
    assert list(c.inputs) == list(c.decoy) and list(c.want) == list(c.decoy_want)
    changed = 0
    for k, a in c.inputs.items():
        d = c.decoy[k]
        assert a.shape == d.shape and a.dtype == d.dtype, k
        changed += not np.array_equal(a, d)
    assert changed >= min(2, len(c.inputs)), "the decoy changes content and lengths"
    for k in c.want:
        share = soc.differing(c, k)
        print(f"{name}: output {k}: the decoy differs in {share:.4f} of the items")
        assert share >= soc.FLOOR, (name, k, share)
    assert set(c.stats) == set(c.decoy_stats)
