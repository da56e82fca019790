"""The resamplers, the likelihood statistics and the pose estimate bit for bit: every case of tests/golden/make_g10_resample_digests.py
recomputed on the device and compared with tests/golden/g10_resample_digests.json, which holds what the kernels wrote before the
resamplers moved into rmcl_amd/csrc/resample.hip and came to share one perturbation and one prefix scan.  The other resampler tests
allow 1e-6 on a perturbed pose; this one allows nothing: a digest that moves means an expression changed its order."""
import importlib.util
import json

import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_g10_resample_digests", golden_path("make_g10_resample_digests.py"))
g10 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g10)

CASES = g10.cases()
with open(golden_path("g10_resample_digests.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_digest_is_the_recorded_one(ra, ctx, name):
    got = CASES[name](ra, ctx)
    assert got == GOLDEN[name], name
