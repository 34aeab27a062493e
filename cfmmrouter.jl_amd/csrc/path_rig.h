// path_rig.h -- internal: the functions of PathRig / TimedPathRig (ctx.h), what the read-only path entries -- abi_quote_path.cpp,
// abi_size_path.cpp, abi_split_paths.cpp, host-pointer and _dev forms alike -- do around their one launch.  Host-side only, on
// top of seg_view.h.  A call is: upload_table (which waits for the call before), the entry's own columns, launch, and for a
// host-pointer entry its read-back and ONE synchronisation.
#pragma once

#include "seg_view.h"

namespace cfmm {

// a failed check's message becomes the context's error
inline int refuse(cfmm_ctx* c, int rc, const char* msg) { return rc == CFMM_OK ? rc : fail(c, rc, "%s", msg); }

// The staging is free again, the table may be rewritten: the call before has left the device (`done` sits behind its kernel)
inline int PathRig::wait_previous(cfmm_ctx* c)
{
    if (in_flight) HIP_TRY(c, hipEventSynchronize(done.get()));
    in_flight = false;
    return CFMM_OK;
}

// The staging grown to the call's layout (the entry's of stage_layout.h, with a `table` column), then table -> staging ->
// device in stream order.  The table is REBUILT FROM THE SEGMENTS' CURRENT ADDRESSES (seg_view.h) on every call:
// cfmm_update_reserves, cfmm_pools_set_ticks and tick compaction swap UniV3 arrays, and a table kept across calls would hold a
// freed address.  It is a line per segment.
template <class Layout>
int PathRig::upload_table(cfmm_ctx* c, const Layout& lay, int32_t& nrec_out)
{
    const size_t nrec = table_records(c);
    int rc;
    if ((rc = wait_previous(c)) || (rc = stage.grow(c, lay.l.words(), false)) || (rc = table.grow(c, nrec)) ||
        (rc = done.create(c, hipEventDisableTiming)))
        return rc;
    PathSeg* t = reinterpret_cast<PathSeg*>(lay.table.in(stage.host()));
    build_table(c, t, [](const Segment& s, size_t) { return path_seg(s); });
    HIP_TRY(c, hipMemcpyAsync(table.get(), t, nrec * sizeof(PathSeg), hipMemcpyHostToDevice, c->stream));
    nrec_out = (int32_t)nrec;
    return CFMM_OK;
}

// go(e0, e1) launches the entry's kernel between the events of pair 0 of `ev` (null unless "time_kernels"); `done` behind it
template <class Launch>
int PathRig::launch(cfmm_ctx* c, EventPairs& ev, const char* what, const Launch& go)
{
    const bool timed = c->opt_time_kernels != 0;
    int rc;
    if (timed && (rc = ev.ensure(c, 1)) != CFMM_OK) return rc;
    const hipError_t e = go(ev.start(0, timed), ev.stop(0, timed));
    if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    HIP_TRY(c, hipEventRecord(done.get(), c->stream));
    in_flight = true;
    return CFMM_OK;
}

// "size_ns" / "split_ns": after a timed _dev call the span is not known until the kernel has run -- the read waits for it and
// stores it, the one thing a getter changes
inline int TimedPathRig::read_ns(cfmm_ctx* c, int64_t* value)
{
    if (dev_timed) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(ev.stop(0)));
        if (const int rc = ev.elapsed_ns(c, 0, 1, ns)) return rc;
        dev_timed = false;
    }
    *value = ns;
    return CFMM_OK;
}

} // namespace cfmm
