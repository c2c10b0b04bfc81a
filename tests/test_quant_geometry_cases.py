"""The batches of tests/quant_geometry_cases.py hold what the GPU tests rely on, from the CPU
oracles alone (needle's restatement for the rows, quant_oracle for the classes): the planted
kinds, the edits at every multiple of 256 columns and at both ends, the share of modified reads,
every class reached, the read lengths that fix the stride."""
import numpy as np
import pytest

from tests import quant_geometry_cases as qc
from tests.test_gpu_quant import PARAMS

CASES = [(qc.full, La, 0) for La in qc.FULL + (2100,)] + [(qc.short, La, 0) for La in qc.SHORT] + \
        [(qc.full, 4952, 32), (qc.full, 4953, 32)]


@pytest.mark.parametrize("fn,La,n", CASES, ids=["%s_%d" % (f.__name__, La) for f, La, _ in CASES])
def test_batch_conditions(fn, La, n):
    case = fn(La, n)
    assert case.n == (n or qc.batch_size(La))
    lens = np.array([len(r) for r in case.reads])
    if fn is qc.full:
        assert lens.max() == La + qc.PAD
    else:
        assert lens.max() == qc.SHORT_MAX and lens.min() >= 80
    rows = qc.oracle_rows(fn, La, n)
    assert int(rows.lens.max()) <= (qc.full_stride(La) if fn is qc.full else qc.short_stride(La))
    refs = {p: qc.oracle_reference(fn, La, p, n)[1] for p in PARAMS}
    fig = qc.conditions(case, rows, refs)
    assert all(len(v) >= qc.KIND_MIN for v in fig["over"].values())


def test_batch_sizes_and_multiples():
    assert [qc.batch_size(L) for L in (400, 1024, 1025, 2100, 2101, 4952)] == [1024, 1024, 256, 256, 64, 64]
    assert qc.multiples(400) == [256] and qc.multiples(580) == [256, 512] and len(qc.multiples(4952)) == 19
    assert qc.full_stride(1393) == 2832 and qc.short_stride(1572) == 1872
