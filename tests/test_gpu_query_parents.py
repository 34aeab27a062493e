"""cfmm_quote, cfmm_quote_out, cfmm_swap and cfmm_swap_out on multi-device parents of 2 and of 8 shards -- with 8, some
shards of every segment are empty -- against the single-device context of the same pools: answers, statuses, the refusal
count and the state the swaps leave, bit for bit, with idx absent and with an unordered idx that repeats a row.  A market of
12 pools: the test runs in a second or two."""
import numpy as np
import pytest

import cfmmrouter_amd as cr
from cfmmrouter_amd import synth
from test_gpu_quote import typical_queries

pytestmark = pytest.mark.gpu

NTOK = 16
DEVICES = (0, [0, 0], [0] * 8)
IDX = ([3, 0, 4, 3, 1], [2, 0, 2, 1], [1, 3, 0, 1])          # per segment: unordered, one row twice


def market():
    return [synth.product_pools(5, NTOK, seed=301), synth.weighted_pools(3, NTOK, 3, seed=302),
            synth.univ3_ragged_pools(4, NTOK, min_ticks=3, max_ticks=3, seed=303)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def calls(batches):
    """per segment the two calls of a test: (seg, amounts, coin_in, coin_out, idx) with idx None, then IDX"""
    out = []
    for seg, b in enumerate(batches):
        ci, co, a = typical_queries(b, len(b), seed=40 + seg)
        rows = np.array(IDX[seg], dtype=np.int64)
        out.append((seg, a, ci, co, None))
        out.append((seg, 0.5 * a[rows], ci[rows], None if co is None else co[rows], rows))
    return out


@pytest.mark.parametrize("entry", ("quote", "quote_out", "swap", "swap_out"))
def test_parents_of_2_and_8_shards_answer_and_move_as_the_single_device_context(entry):
    batches = market()
    assert [len(b) for b in batches] == [5, 3, 4] and batches[1].Ai.shape[1] == 3
    assert np.all(np.diff(batches[2].tick_off) == 3)
    bes = [cr.DeviceBackend(NTOK, batches, device=d) for d in DEVICES]
    try:
        one = bes[0].ctx
        swaps, exact_out = entry.startswith("swap"), entry.endswith("_out")
        for seg, a, ci, co, idx in calls(batches):
            # exact output: ask for 0.3 of what the single-device context quotes for the amounts NOW (the same wanted amounts
            # go to every context; on equal states it is the same number anyway)
            given = 0.3 * one.quote(seg, a, ci, co, idx) if exact_out else a
            got = []
            for be in bes:
                if entry == "swap_out":
                    ans, st = be.ctx.swap_out(seg, given, ci, co, idx, status=True)
                    got.append((ans, st, be.ctx.get_option("swap_refused")))
                else:
                    ans = getattr(be.ctx, entry)(seg, given, ci, co, idx)
                    got.append((ans, np.zeros(len(ans), dtype=np.int32), be.ctx.get_option("swap_refused") if swaps else 0))
            ref = got[0]
            assert np.all(np.isfinite(ref[0])) and np.any(ref[0] > 0) and len(ref[0]) == len(ci)
            for ans, st, refused in got[1:]:
                np.testing.assert_array_equal(bits(ans), bits(ref[0]))
                np.testing.assert_array_equal(st, ref[1])
                assert refused == ref[2]
        # every pool in the same state everywhere: a dense quote of every segment, both directions of the first two coins
        for seg, b in enumerate(batches):
            ci, co, a = typical_queries(b, len(b), seed=60 + seg)
            for flip in (False, True):
                cin = ((ci + 1) % b.Ai.shape[1]).astype(np.int32) if flip else ci
                cout = None if co is None else ((cin + 1) % b.Ai.shape[1]).astype(np.int32)
                dense = [be.ctx.quote(seg, a, cin, cout) for be in bes]
                assert np.all(np.isfinite(dense[0]))
                for d in dense[1:]:
                    np.testing.assert_array_equal(bits(d), bits(dense[0]))
        if swaps:      # ... and it is not the state of the upload
            fresh = cr.DeviceBackend(NTOK, batches, device=0)
            try:
                ci, co, a = typical_queries(batches[0], 5, seed=60)
                assert np.any(bits(fresh.ctx.quote(0, a, ci, co)) != bits(one.quote(0, a, ci, co)))
            finally:
                fresh.close()
    finally:
        for be in bes:
            be.close()
