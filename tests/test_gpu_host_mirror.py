"""The host mirror's index maps on the real DeviceBackend: a router built from an interleaved list of all six pool kinds and
one plugin pool hands back, pool for pool and bit for bit, the trades of a router built from the same pools already packed
(`_segments_of`'s batches), before and after update_pools_."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
import host_mirror_record as rec
from cfmmrouter_amd.router import _segments_of

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same_trades(r, q, order, host):
    Dr, Lr, Dq, Lq = r.Δs, r.Λs, q.Δs, q.Λs
    assert len(Dr) == len(order) + len(host) and len(Dq) == len(order)
    for k, i in enumerate(order):
        np.testing.assert_array_equal(bits(Dr[i]), bits(Dq[k]), err_msg=f"Δ of pool {i}")
        np.testing.assert_array_equal(bits(Lr[i]), bits(Lq[k]), err_msg=f"Λ of pool {i}")
    for min_value in (-np.inf, 0.0):
        ir, ar, br, vr = cr.active_trades(r, min_value)
        iq, aq, bq, vq = cr.active_trades(q, min_value)
        assert np.all(np.diff(ir) > 0) and np.all(np.diff(iq) > 0)
        got = {int(i): (bits(a).tolist(), bits(b).tolist(), bits(v).tolist()) for i, a, b, v in zip(ir, ar, br, vr) if i not in host}
        want = {int(order[k]): (bits(a).tolist(), bits(b).tolist(), bits(v).tolist()) for k, a, b, v in zip(iq, aq, bq, vq)}
        assert got == want and (min_value != -np.inf or len(got) >= 3)


@pytest.mark.timeout(60)
def test_router_order_equals_packed_order_through_the_layout():
    n = rec.N_TOKENS
    make = lambda: [p for i, p in enumerate(rec.mixed_pools()) if i != 7]          # 14 pools, the plugin pool first
    pools = make()
    packed, order, host = _segments_of(make())
    assert host == [0] and sorted(order.tolist()) == list(range(1, 14)) and not np.array_equal(order, np.arange(1, 14))
    assert [(b.kind, b.n_coins) for b in packed] == [(p.kind, len(p.Ai)) for p in (pools[2], pools[6], pools[4], pools[5], pools[8], pools[3], pools[7], pools[1])]
    obj = cr.LinearNonnegative(np.ones(n))
    r, q = cr.Router(obj, pools, n), cr.Router(obj, packed, n)
    try:
        v = 1.0 + 0.1 * np.arange(n)
        cr.find_arb_(r, v)
        cr.find_arb_(q, v)
        assert_same_trades(r, q, order, host)
        # one pool of each kind (UniV3: a bare price and a new ladder in one segment), by its position in each router
        new = {2: [101.0, 202.0], 6: [31.0, 41.0], 5: [1002.0, 1003.0], 3: [51.0, 61.0, 71.0, 81.0],
               1: ([102.0, 103.0, 98.0], 1400.0, 3.8e6), 10: 0.85, 4: rec.LADDER}
        where = {int(i): k for k, i in enumerate(order)}
        cr.update_pools_(r, new)
        cr.update_pools_(q, {where[i]: s for i, s in new.items()})
        for i in new:
            assert rec.digest(rec.pool_fields(r.cfmms[i])) == rec.digest(rec.pool_fields(q.cfmms[where[i]])), i
        assert all(np.all(x == 0.0) for x in q.Δs + r.Δs)                            # the old market's trades are gone
        cr.find_arb_(r, v)
        cr.find_arb_(q, v)
        assert_same_trades(r, q, order, host)
        assert r.cfmms[4].current_tick == int(np.count_nonzero(rec.LADDER[1] >= rec.LADDER[0])) and r.cfmms[10].current_price == 0.85
    finally:
        r.close()
        q.close()
