"""Lifetime of the binding's objects: an engine or cache created on a context
holds a native handle that points into it, and its destroy call reads the
context.  Whatever order close() / the garbage collector takes them in, the
context closes what was created on it first."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def spray():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import spray_amd
    return spray_amd


def test_context_closes_its_engines_first(spray):
    from spray_amd import insitu
    rt = spray.RtContext(0)
    rt.domain_bounds(np.array([[0, 0, 0, 1, 1, 1]], np.float32))
    rt.set_owners(np.zeros(1, np.int32))
    eng = insitu.InsituEngine(rt, 1, 0, transport="host")
    ooc = spray.OocCache(rt, 1)
    assert eng.h and ooc.h
    rt.close()  # the context first: it takes its engine and cache along
    assert eng.h is None and ooc.h is None and rt.h is None
    eng.close()
    ooc.close()


def test_unreachable_group_is_finalized_in_order(spray):
    """An engine and its context dropped together (what a failed call inside
    pytest.raises leaves behind) and finalized by the collector."""
    import torch
    from spray_amd import insitu

    def leak():
        rt = spray.RtContext(0)
        rt.domain_bounds(np.array([[0, 0, 0, 1, 1, 1]], np.float32))
        rt.set_owners(np.zeros(1, np.int32))
        eng = insitu.InsituEngine(rt, 1, 0, transport="host")
        return eng.h

    for _ in range(4):
        assert leak()
    gc.collect()
    # no HIP error is left pending for the next kernel launch of the process
    assert int(torch.zeros(4, dtype=torch.int32, device="cuda").sum().item()) == 0
