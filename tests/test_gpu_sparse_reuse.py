"""One context reused across sparse fits and likelihoods of changing shapes, kernels, types and
modes (tests/sparse_reuse_ref.py): every call gives the bits of the same call on a fresh context,
and the oracle's values at the suite's tolerances.

Each scenario creates its own contexts: the session's `ctx` has whatever history the collection
order gave it, and is not the context under test."""
import pytest

from tests import sparse_reuse_ref as R

pytestmark = pytest.mark.gpu


def _context():
    import gpr_amd
    return gpr_amd.Context(0)


@pytest.mark.parametrize("name", list(R.SCENARIOS))
def test_sparse_reuse(name):
    R.run(name, _context, verbose=True)
