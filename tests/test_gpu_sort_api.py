"""``orderBy`` / ``sort`` / ``sortWithinPartitions`` / ``ORDER BY`` on the device session: every case
of ``test_sort_host.py`` collects the CPU engine's rows, row for row."""
import pytest
import torch

from test_sort_host import api_results, lab_frame
from net.jgp.labs.sparkdq4ml_amd.sql import functions as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cpu_results():
    """The CPU engine's answers (computed before the device session exists)."""
    from net.jgp.labs.sparkdq4ml_amd import SparkSession

    s = SparkSession.getActiveSession()
    if s is not None:
        s.stop()
    s = SparkSession.builder().appName("test").master("cpu").getOrCreate()
    try:
        return api_results(s), [tuple(r) for r in lab_frame(s).collect()]
    finally:
        s.stop()


def test_every_case_equals_the_cpu_engine(cpu_results, gpu_session):
    want_all, _ = cpu_results
    got = api_results(gpu_session)
    assert sorted(got) == sorted(want_all)
    for name, want in want_all.items():
        assert repr(got[name]) == repr(want), name  # exact, NaN and null cells included
    assert len(got["lab_counts"]) > 10


def test_device_scan_filtered_then_sorted(cpu_results, gpu_session):
    _, rows = cpu_results
    df = lab_frame(gpu_session).filter("price > 100")
    t = df._table()
    assert t.device.type == "cuda" and t.sel is not None and t.nrows == len(rows)  # the selection vector is kept ...
    s = df.orderBy(F.desc("price"), "guest")
    st = s._table()  # ... and reaches the sort kernels as it is: the result is compact and on the device
    assert st.device.type == "cuda" and st.sel is None and st.nrows == sum(1 for r in rows if r[1] > 100)
    for c in st.columns:
        assert torch.is_tensor(c.values) and c.values.is_cuda
    assert [tuple(r) for r in s.collect()] == sorted([r for r in rows if r[1] > 100], key=lambda r: (-r[1], r[0]))
    top = s.limit(5)
    assert [tuple(r) for r in top.collect()] == sorted([r for r in rows if r[1] > 100], key=lambda r: (-r[1], r[0]))[:5]
