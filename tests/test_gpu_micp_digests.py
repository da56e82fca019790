"""Every MICP entry point bit for bit: each case of tests/golden/make_g11_micp_digests.py recomputed on the device -- the loop form it
ended in proven from micp_fast_info -- and compared with tests/golden/g11_micp_digests.json, which holds what the kernels wrote before
they moved into rmcl_amd/csrc/micp.hip and came to share one fold hand-over, one mask scan and one point-to-plane accumulate.  The other
MICP tests allow 1e-6 on a pose; this one allows nothing: a digest that moves means an expression or a sum changed its order."""
import importlib.util
import json

import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_g11_micp_digests", golden_path("make_g11_micp_digests.py"))
g11 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g11)

CASES = g11.cases()
with open(golden_path("g11_micp_digests.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_digest_is_the_recorded_one(ra, ctx, name):
    got = CASES[name](ra, ctx)
    assert got == GOLDEN[name], name
