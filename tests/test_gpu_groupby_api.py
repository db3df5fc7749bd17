"""``groupBy`` / ``agg`` / ``distinct`` / ``dropDuplicates`` / ``GROUP BY`` on the device session:
every case of ``test_groupby_host.py`` collects the CPU engine's rows, row for row."""
import math

import pytest
import torch

from test_groupby_host import api_results, lab_frame, lab_rows
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
        return api_results(s)
    finally:
        s.stop()


def test_every_case_equals_the_cpu_engine(cpu_results, gpu_session):
    got = api_results(gpu_session)
    assert sorted(got) == sorted(cpu_results)
    for name, want in cpu_results.items():
        assert repr(got[name]) == repr(want), name  # exact, NaN and null cells included
    assert len(got["count"]) == len({g for g, _ in lab_rows()})


def test_device_scan_filtered_then_grouped(gpu_session):
    df = lab_frame(gpu_session).filter("price > 50")
    t = df._table()
    assert t.device.type == "cuda" and t.sel is not None and t.nrows == len(lab_rows())  # selection vector kept
    r = df.groupBy("guest").agg(F.count("*"), F.sum("price"), F.min("price"), F.avg("guest"))
    rt = r._table()
    assert rt.device.type == "cuda" and rt.sel is None
    for c in rt.columns:  # the result columns live on the device
        assert torch.is_tensor(c.values) and c.values.is_cuda
    by = {}
    for g, p in lab_rows():
        if p > 50:
            by.setdefault(g, []).append(p)
    assert [tuple(x) for x in r.collect()] == [(g, len(by[g]), math.fsum(by[g]), min(by[g]), float(g)) for g in sorted(by)]
    kept = df.dropDuplicates(["guest"])
    kt = kept._table()
    assert kt.nrows == t.nrows and kt.sel.is_cuda and int(kt.sel.sum()) == len(by)  # no row moved
    first = {}
    for g, p in lab_rows():
        if p > 50:
            first.setdefault(g, p)
    assert [tuple(x) for x in kept.collect()] == list(first.items())
