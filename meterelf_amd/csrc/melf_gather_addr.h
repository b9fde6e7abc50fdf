// Address arithmetic of k_gather_rows (k_gather.hip): which rows of which run a wave copies, and for every 16-byte piece of a
// destination row the source offset, the bytes it holds and the loads that fetch them.  Plain C++, the sibling of melf_prep_addr.h:
// the kernel computes its addresses with these functions, and tests/stage_runs_main.cpp executes the same functions on the CPU
// against frames of exact extent.  Source offsets count BYTES from a frame's pointer, destination offsets from its staged frame.
// k_plane_rows, the same copy from one pointer per PLANE, adds wave_run and plane_rows (tests/plane_runs_main.cpp executes those).
//
// A destination row starts on a 64-byte boundary, so piece p of a row is the 16 aligned bytes [16 p, 16 p + 16) of it.  A piece that
// lies wholly inside the row's bytes is one 16-byte load at whatever alignment the source row has; the last piece of a row whose
// length is no multiple of 16 holds 1 .. 15 bytes and is fetched with loads of 8, 4, 2 and 1 bytes -- the binary digits of its
// length --, so that exactly the row's bytes are read and nothing behind them.  (Pieces are cut at the destination's alignment: there
// is no head piece.)  The bytes of the last piece behind the row's end are written as zeros: they lie in the row's pitch padding.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "melf_stage_plan.h"

#if defined(__HIPCC__)
#define MELF_GATHER_FN __host__ __device__ __forceinline__
#else
#define MELF_GATHER_FN inline
#endif

namespace melf {
namespace gather {

constexpr int PIECE = 16;            // bytes of a piece: one 16-byte store
constexpr int ROWS_PER_WAVE = 8;     // rows of one run a wave copies: 47 pieces a row of a 250-pixel BGR crop, 6 per lane
constexpr int WAVES_PER_BLOCK = 4;

// waves of one frame: the runs' blocks of ROWS_PER_WAVE rows, run after run
MELF_GATHER_FN uint32_t run_waves(const RowRun& r) { return (r.rows + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE; }
MELF_GATHER_FN uint32_t frame_waves(const RowRuns& rr)
{
    uint32_t t = 0;
    for (int k = 0; k < STAGE_MAX_RUNS; ++k)
        if (k < rr.count) t += run_waves(rr.run[k]);
    return t;
}
// The run and the first row of wave w of a frame (w < frame_waves): no indexing of the by-value runs with a runtime value (that
// would put them into the private segment), three selects
struct WaveRows {
    RowRun run;
    uint32_t row0, nrows;   // rows [row0, row0 + nrows) of the run
};
MELF_GATHER_FN WaveRows wave_rows(const RowRuns& rr, uint32_t w)
{
    const uint32_t w0 = run_waves(rr.run[0]), w1 = rr.count > 1 ? run_waves(rr.run[1]) : 0;
    const int k = w < w0 ? 0 : (w < w0 + w1 ? 1 : 2);
    const uint32_t b = k == 0 ? w : (k == 1 ? w - w0 : w - w0 - w1);
    WaveRows o;
    // (masks, not ?: -- the compiler turns a chain of selects between the elements of one array back into an indexed load)
    const uint64_t m0 = 0 - (uint64_t)(k == 0), m1 = 0 - (uint64_t)(k == 1), m2 = 0 - (uint64_t)(k == 2);
#define MELF_GATHER_SEL(field) o.run.field = (decltype(o.run.field))((rr.run[0].field & m0) | (rr.run[1].field & m1) | (rr.run[2].field & m2))
    MELF_GATHER_SEL(src_off); MELF_GATHER_SEL(dst_off); MELF_GATHER_SEL(src_pitch); MELF_GATHER_SEL(dst_pitch);
    MELF_GATHER_SEL(row_bytes); MELF_GATHER_SEL(rows);
#undef MELF_GATHER_SEL
    o.row0 = b * ROWS_PER_WAVE;
    o.nrows = o.run.rows - o.row0 < (uint32_t)ROWS_PER_WAVE ? o.run.rows - o.row0 : (uint32_t)ROWS_PER_WAVE;
    return o;
}

// k_plane_rows (a frame's planes in separate allocations): the index of wave w's run -- the plane slot its rows are read from --, as
// wave_rows finds it
MELF_GATHER_FN uint32_t wave_run(const RowRuns& rr, uint32_t w)
{
    const uint32_t w0 = run_waves(rr.run[0]), w1 = rr.count > 1 ? run_waves(rr.run[1]) : 0;
    return w < w0 ? 0u : (w < w0 + w1 ? 1u : 2u);
}
// ... and the wave's rows with the run's source offset counted from that plane's own pointer, of which `extent` bytes are readable
// (PlaneSplit: melf_stage_plan.h); the same masks as wave_rows, for the same reason
struct PlaneRows {
    WaveRows wr;       // wr.run.src_off: from the pointer of plane slot k
    uint32_t k;
    uint64_t extent;   // of plane slot k
};
MELF_GATHER_FN PlaneRows plane_rows(const RowRuns& rr, const PlaneSplit& ps, uint32_t w)
{
    PlaneRows o;
    o.wr = wave_rows(rr, w);
    o.k = wave_run(rr, w);
    const uint64_t m0 = 0 - (uint64_t)(o.k == 0), m1 = 0 - (uint64_t)(o.k == 1), m2 = 0 - (uint64_t)(o.k == 2);
    o.wr.run.src_off = (ps.src_off[0] & m0) | (ps.src_off[1] & m1) | (ps.src_off[2] & m2);
    o.extent = (ps.extent[0] & m0) | (ps.extent[1] & m1) | (ps.extent[2] & m2);
    return o;
}

// pieces of a row
MELF_GATHER_FN uint32_t row_pieces(uint32_t row_bytes) { return (row_bytes + PIECE - 1) / PIECE; }

// Piece `piece` of row `row` of a run: where its bytes lie in the frame and in the staged frame, and how many it holds -- 16: the
// full path, one 16-byte load; 1 .. 15: the tail path, loads of the widths tail_width gives
struct Piece {
    uint64_t src_off, dst_off;
    uint32_t bytes;
};
MELF_GATHER_FN Piece piece_of(const RowRun& r, uint32_t row, uint32_t piece)
{
    Piece p;
    p.src_off = r.src_off + (uint64_t)row * r.src_pitch + (uint64_t)piece * PIECE;
    p.dst_off = r.dst_off + (uint64_t)row * r.dst_pitch + (uint64_t)piece * PIECE;
    const uint32_t left = r.row_bytes - piece * PIECE;
    p.bytes = left < (uint32_t)PIECE ? left : (uint32_t)PIECE;
    return p;
}
// the piece's bytes are inside what may be read of the frame (always, for the runs of a plan made from the frame's checked
// descriptor; the kernel drops a piece that is not)
MELF_GATHER_FN bool piece_readable(const Piece& p, uint64_t extent) { return p.src_off + p.bytes <= extent; }

// Tail path: the load of width w (8, 4, 2, 1) is made if bit w of the piece's byte count is set, at this offset inside the piece:
// the wider loads come first
MELF_GATHER_FN bool tail_has(uint32_t bytes, uint32_t w) { return (bytes & w) != 0; }
MELF_GATHER_FN uint32_t tail_at(uint32_t bytes, uint32_t w) { return bytes & ~(2 * w - 1) & 15u; }

}  // namespace gather
}  // namespace melf
