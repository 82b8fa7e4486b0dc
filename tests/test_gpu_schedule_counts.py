"""What each factor schedule issues, as mpf_stats counts it (panels, schedule, update launches, flops, bytes, one-pass blocks,
info), against the values recorded by tools/schedule_counts.py in tests/golden/schedule_counts.json: the bit tests do not see a
dropped count_gemm or a changed number of launches.  The lane split and the pair conditions depend on the CU count, so the fixture
holds for the device it was recorded on."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("schedule_counts", os.path.join(ROOT, "tools", "schedule_counts.py"))
SC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SC)
with open(os.path.join(ROOT, "tests", "golden", "schedule_counts.json")) as _f:
    GOLD = json.load(_f)


def test_the_fixture_covers_every_case():
    assert sorted(GOLD["cases"]) == sorted(c[0] for c in SC.cases())
    assert all(sorted(v) == sorted(SC.FIELDS) for v in GOLD["cases"].values())


@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c[0])
def test_schedule_counts_match_the_recorded_ones(mpf, case):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != GOLD["num_cus"]:
        pytest.skip(f"fixture recorded on a device with {GOLD['num_cus']} CUs, this one has {cus}")
    name, n, nb, trailing, opts = case
    got = SC.run_case(mpf, n, nb, trailing, opts)
    want = GOLD["cases"][name]
    print(name, got)
    assert got == want, {f: (got[f], want[f]) for f in SC.FIELDS if got[f] != want[f]}
