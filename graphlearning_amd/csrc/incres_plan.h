// What the host decides for the grow loop of INCRES clustering (glx_incres_step, incres.hip; reference clustering.py:356-358):
//     while np.min(F) == 0:  F = P*F
// No HIP header: tests/test_incres_host.py builds it on the host (tests/incres_plan_host.cpp), where a plain loop stands in for the
// kernels and runs the same chunked schedule.
//
// The schedule.  The planted state is iterate 0, one sweep makes iterate t + 1 of iterate t.  Behind every iterate a census writes one
// flag -- does the iterate hold a 0.0 among its real columns? -- and the iterate's row-wise first-maximum index into the label buffer of
// the iterate's SLOT.  The host enqueues a chunk of (sweep, census) pairs and reads the chunk's flags once: slot r of a chunk that
// starts behind `done` sweeps belongs to iterate done + r; slot 0 is used by the first chunk of a grow loop only (the planted state
// itself).  The first slot without a zero ends the loop: its iterate number is the reference's sweep count, its label buffer the
// harvest.  Sweeps enqueued behind it are wasted, not wrong -- the next plant overwrites the state.
//
// The chunk length never changes a result: it decides how many sweeps are wasted and how often the host waits.  First chunk of a
// grow loop: the count of the loop before plus a margin (the seeds per cluster grow from one outer iteration to the next, so the counts
// fall, or rise by one: profiles/incres.txt), a fixed guess for the first loop; later chunks start short and double, so a loop that is
// much longer than the one before costs a number of waits that grows with the logarithm of its length.  All of them at most
// INCRES_MAX_CHUNK, so the flags and label buffers have a fixed size: device memory grows neither with T nor with the sweep count.
//
// The cap.  The reference's loop does not end on a disconnected graph, on a bipartite one (a path without self loops) or when values
// underflow to 0 before they arrive; the device version gives up after max_grow sweeps of one grow loop (INCRES_CAPPED).  The iterate
// behind exactly max_grow sweeps is still tested: a loop that needs max_grow sweeps succeeds.
#pragma once
#include <cstdint>

static const int INCRES_MAX_COLS = 256;       // clusters per handle: the record layout's column cap
static const int INCRES_MAX_CHUNK = 64;       // sweeps per chunk at most: 65 flags and label buffers per handle
static const int INCRES_FIRST_CHUNK = 16;     // the first grow loop of a handle: nothing is known yet
static const int INCRES_MARGIN = 1;           // first chunk of a later loop: the count before + this
static const int INCRES_NEXT_CHUNK = 4;       // the second chunk of a loop; every further one twice the one before
static const int INCRES_CAPPED = 1;           // incres_grow: max_grow sweeps and still a zero

struct IncresPlan {
  int forced = 0;          // > 0: every chunk has this length (tests; clamped like the others)
  int margin = 0, next = 0;      // > 0: in the place of INCRES_MARGIN / INCRES_NEXT_CHUNK (measurements)
  int64_t prev = -1;       // sweep count of the grow loop before (-1: none yet)
  int64_t loops = 0, chunks = 0, enqueued = 0, counted = 0;      // what the schedule cost so far
  // sweeps of the next chunk of a loop that has `nth` chunks and `done` sweeps behind it (done < max_grow): 1 .. min(INCRES_MAX_CHUNK,
  // max_grow - done)
  int chunk_len(int64_t done, int64_t max_grow, int64_t nth) const {
    int64_t len;
    if (forced > 0) len = forced;
    else if (nth > 0) len = nth > 6 ? INCRES_MAX_CHUNK : (int64_t)(next > 0 ? next : INCRES_NEXT_CHUNK) << (nth - 1);
    else len = prev < 0 ? INCRES_FIRST_CHUNK : prev + (margin > 0 ? margin : INCRES_MARGIN);
    if (len > INCRES_MAX_CHUNK) len = INCRES_MAX_CHUNK;
    if (len > max_grow - done) len = max_grow - done;
    return len < 1 ? 1 : (int)len;
  }
};

// One grow loop on the planted state.  Ops:
//   int begin_chunk(int first, int len)        the flags of slots first .. len are cleared
//   int census(int slot)                       flag and labels of the current iterate -> slot
//   int sweep()                                the current iterate <- P * the current iterate
//   int read_flags(int first, int len, const int32_t** flags)      waits; (*flags)[r] != 0: the iterate of slot r holds a zero
// each returning 0 or an error code that ends the loop and is returned as it is (negative: the library's codes).  0: *sweeps and *slot
// are set; INCRES_CAPPED: *sweeps = max_grow.
template <class Ops>
int incres_grow(IncresPlan& plan, int64_t max_grow, Ops& ops, int64_t* sweeps, int* slot) {
  int64_t done = 0;
  ++plan.loops;
  for (int64_t nth = 0;; ++nth) {
    const int first = done == 0 ? 0 : 1;
    const int len = plan.chunk_len(done, max_grow, nth);
    int rc = ops.begin_chunk(first, len);
    if (rc) return rc;
    if (first == 0 && (rc = ops.census(0))) return rc;
    for (int r = 1; r <= len; ++r) {
      if ((rc = ops.sweep())) return rc;
      if ((rc = ops.census(r))) return rc;
    }
    const int32_t* flags = nullptr;
    if ((rc = ops.read_flags(first, len, &flags))) return rc;
    ++plan.chunks;
    plan.enqueued += len;
    for (int r = first; r <= len; ++r)
      if (!flags[r]) {
        *sweeps = done + r;
        *slot = r;
        plan.prev = done + r;
        plan.counted += done + r;
        return 0;
      }
    done += len;
    if (done >= max_grow) {
      *sweeps = done;
      *slot = -1;
      plan.counted += done;
      return INCRES_CAPPED;
    }
  }
}
