"""A profiling scope that is left by an error return still records its stop event (csrc/common.h: ProfScope)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_failed_exchange_closes_its_profiling_scope():
    """A halo exchange of a partitioned level whose communication callback returns non-zero ONCE: the call raises (an error code
    from the host side, nothing faults), the same call then succeeds, and the event table is still readable --
    ``prof_get()`` returns, and counts one COMM scope per exchange call, the failed one included.  With the hand-written
    begin / end pairs the failed call returned between the two: its start event stayed counted without a stop event, and the
    next ``alfi_prof_get_level`` asked hipEventElapsedTime for a pair that was never completed."""
    from alfi_amd import hip
    from alfi_amd.dist import CommFn
    from alfi_amd.problem import BSR
    rng = np.random.default_rng(3)
    bs, n_own, n_ghost = 3, 500, 130
    nb = n_own + n_ghost
    A = BSR(nb, nb, bs, np.arange(nb + 1, dtype=np.int32), np.arange(nb, dtype=np.int32), np.tile(np.eye(bs), (nb, 1, 1)))
    ctx = hip.Context(0)
    try:
        calls = []

        def callback(user, op, level_id, offset, count):
            calls.append(op)
            return 7 if len(calls) == 1 else 0          # fails once

        cb = CommFn(callback)
        dred = ctx.vec(64)                              # the buffer all-reduces would use (>= 2 * RED_MAXV doubles)
        ctx.set_comm(cb, dred.ptr.value, 64)
        ctx.prof_enable(True)
        L = hip.Level(ctx, A, np.zeros(0, dtype=np.int32))
        send_nodes = rng.integers(0, n_own, n_ghost).astype(np.int32)
        L.set_partition(n_own, True, send_nodes, None, None, n_ghost)
        dv = ctx.vec(rng.standard_normal(nb * bs))
        ctx.prof_reset()
        with pytest.raises(hip.AlfiHipError, match="communication callback failed"):
            L.halo_forward(dv)
        L.halo_forward(dv)
        ctx.sync()
        assert len(calls) == 2
        prof = ctx.prof_get()                           # must not raise
        assert prof["COMM"][1] == 2                     # both scopes, each with its stop event
        assert prof["COMM"][0] >= 0.0
        assert all(cnt == 0 for name, (ms, cnt) in prof.items() if name != "COMM")
    finally:
        ctx.close()
