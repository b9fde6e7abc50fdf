// Address arithmetic of k_narrow_rows and its two list siblings (k_narrow.hip) and of the host packers of melf_process_wide*: which
// samples of a wide frame (16-bit or floating-point samples, melf_narrow.h narrows one) make which 16-byte piece of the staged frame.
// Plain C++, the sibling of melf_gather_addr.h, on which it stands: tests/wide_narrow_main.cpp executes the same functions on the CPU
// against frames of exact extent, tests/wide_list_main.cpp against listed frames and planes of exact extent (the end of this file:
// a wide frame's planes in separate allocations).
//
// The staged frame is the one the plan of the 8-bit batch of the same geometry gives (check_wide leaves that batch, every offset
// and pitch counted in SAMPLES): packed_plan / planar_plan of melf_stage_plan.h.  A staged byte is one narrowed sample, so a run's
// src_off, src_pitch and row_bytes count samples of the source, and times the sample size they are its bytes.  The launch shape is
// that of k_gather_rows: one wave per (frame, run, block of ROWS_PER_WAVE rows) -- gather::wave_rows --, a lane per 16-byte piece of
// a staged row: piece p of a row holds the row's samples [16 p, 16 p + 16).  A piece that lies wholly inside the row is 32 (64:
// float32) consecutive source bytes, fetched with 16-byte loads at whatever alignment the source has; the row's last piece, of
// 1 .. 15 samples, takes its samples one by one, so that nothing behind the row's last sample is loaded.  The bytes of the last
// piece behind the row's end are written as zeros: they lie in the row's pitch padding.
//
// Which scale and offset a sample takes is a matter of its position (narrow::Rule): sample j of a packed row is sample j mod channels
// of its pixel -- a run starts at a pixel's first sample --, and piece p starts at position 16 p mod channels; every sample of a
// planar run has the position of its plane, the run's index.
#pragma once
#include "melf_gather_addr.h"
#include "melf_narrow.h"

namespace melf {
namespace narrow {

constexpr int PIECE = gather::PIECE;   // samples of a piece = its staged bytes

// The plan of a checked wide batch: the staged frame (what the reading kernels take, bytes) and the runs (the source's, in samples)
inline StagePlan wide_plan(const WideBatch& wb, const Crop& cr) { return stage_plan(wb.b, cr); }

// A piece's samples in the source: `count` samples from sample `sample` of the frame (byte sample * ss from its pointer), the first
// of them sample j0 of its row
struct Samples {
    uint64_t sample, dst_off;
    uint32_t count, j0;
};
MELF_GATHER_FN Samples samples_of(const RowRun& r, uint32_t row, uint32_t piece)
{
    const gather::Piece p = gather::piece_of(r, row, piece);
    Samples s;
    s.sample = p.src_off; s.dst_off = p.dst_off; s.count = p.bytes; s.j0 = piece * (uint32_t)PIECE;
    return s;
}
// the samples are inside what may be read of the frame: extent counts samples (always, for the runs of a plan made from the
// frame's checked descriptor; the kernel drops a piece that is not)
MELF_GATHER_FN bool samples_readable(const Samples& s, uint64_t extent) { return s.sample + s.count <= extent; }
// position of a packed piece's first sample in its pixel (channels 3 or 4)
MELF_GATHER_FN uint32_t piece_phase(uint32_t piece, uint32_t channels) { return (piece * (uint32_t)PIECE) % channels; }

// The host packer of melf_process_wide: work item `item` of the plan (stage_item: a block of 32 rows of one run) of the caller's frame
// at `frame` into its staged frame at `staged`, piece by piece as the kernel does it, every sample narrowed on the way
// rows [r0, r1) of run k (run.src_off: samples from src)
inline void pack_run_rows(const uint8_t* src, uint8_t* staged, const RowRun& run, int k, uint32_t r0, uint32_t r1, const Rule& rule, int ss)
{
    const uint32_t ppr = gather::row_pieces(run.row_bytes);
    for (uint32_t y = r0; y < r1; ++y)
        for (uint32_t p = 0; p < ppr; ++p) {
            const Samples s = samples_of(run, y, p);
            narrow_samples(staged + s.dst_off, src + s.sample * (uint64_t)ss, s.count, s.j0, (uint32_t)k, rule);
        }
}
inline void pack_item(const uint8_t* frame, uint8_t* staged, int item, const StagePlan& sp, const Rule& rule, int ss)
{
    int k0, k1;
    uint32_t r0, r1;
    stage_item(sp, item, &k0, &k1, &r0, &r1);
    for (int k = k0; k < k1; ++k) pack_run_rows(frame, staged, sp.runs.run[k], k, r0, r1, rule, ss);
}

// ---- a wide frame's planes in separate allocations (melf_process_wide_plane_list*, k_narrow_plane_rows) ----
// The PlaneSplit of a wide plane list, in SAMPLES: check_wide_plane_list (melf_stage_plan.h) leaves the canonical batch and its
// PlaneList in samples, so run k of the plan starts src_off[k] samples behind plane slot k's own pointer, of which extent[k] samples
// are readable.  The kernel takes a wave's rows through gather::plane_rows of this split and tests every piece with
// samples_readable against that plane's extent.
inline PlaneSplit wide_plane_split(const RowRuns& runs, const PlaneList& pl_in_samples) { return plane_split(runs, pl_in_samples); }
// run k of the plan as it is read from plane slot k's pointer
MELF_GATHER_FN RowRun plane_run(const RowRun& run, const PlaneSplit& split, int k)
{
    RowRun r = run;
    r.src_off = split.src_off[k];
    return r;
}
// The host packer's plane-list form: run k from planes[k] (the frame's three pointers, B / G / R)
inline void pack_item(const void* const* planes, uint8_t* staged, int item, const StagePlan& sp, const PlaneSplit& split, const Rule& rule, int ss)
{
    int k0, k1;
    uint32_t r0, r1;
    stage_item(sp, item, &k0, &k1, &r0, &r1);
    for (int k = k0; k < k1; ++k) pack_run_rows((const uint8_t*)planes[k], staged, plane_run(sp.runs.run[k], split, k), k, r0, r1, rule, ss);
}

}  // namespace narrow
}  // namespace melf
