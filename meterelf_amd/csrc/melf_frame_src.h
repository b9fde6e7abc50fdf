// Frame sources of the dial reader: how the bytes of each frame layout become pixels.  k_dials_body.inc is written once against
// the interface stated above the sources; a kernel wrapper (k_dials.hip) names its source type (`Src`) and hands the body the
// kernel's own arguments of that layout (`sargs`, an Src::Args).  Adding a layout: DESIGN.md, "Adding a layout".
#pragma once
#include "melf_device.h"
#include "melf_internal.h"
#include "melf_y16_addr.h"
#include "melf_p10_addr.h"
#include "melf_p32_addr.h"

namespace melf {

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));

// Host seams.  tests/frame_src_bounds_main.cpp compiles this header as plain C++ and runs the sources on the CPU against buffers of
// exact extent; two constructs have no host form and are the device's own text only in the device compile (__HIP_DEVICE_COMPILE__):
// the scalar-register constraint in load_px3_row, and the 16-byte load of a 4-byte-aligned address (load16), a plain dereference
// on the device, bytes copied on the host (x86 faults on a 16-byte vector load that is not 16-byte aligned).
__device__ __forceinline__ u32x4v load16(const void* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const u32x4v*)p;
#else
    u32x4v v;
    __builtin_memcpy(&v, p, 16);
    return v;
#endif
}

// ---- packed 3-byte pixels, one at a time ----------------------------------------------------------------------------------
// Three bytes of a packed 3-channel pixel with ONE (unaligned) dword load instead of three byte loads: the
// dword starts one byte early (so it never runs past the buffer's end) except at the buffer's very first pixel.
// The top byte of the result is unspecified (every user looks at bytes 0..2 only).
__device__ __forceinline__ uint32_t load_px3(const uint8_t* p, const uint8_t* buffer_start)
{
    const uint32_t back = p == buffer_start ? 0u : 1u;
    uint32_t v;
    __builtin_memcpy(&v, p - back, 4);
    return v >> (8u * back);
}

// The same for a lane's COLUMN of pixels, col + row_off for wave-uniform row offsets: the address arithmetic of
// load_px3 (a 64-bit multiply-add, a 64-bit compare against the buffer's start, a select) cost ten issue slots per window
// row and lane, a tenth of the kernel's vector instructions.  Here the direction is fixed per LANE: the dword starts one
// byte early, except in the lane whose column begins at the buffer's first byte, which reads forward in every row (one
// byte into its right-hand neighbour: inside the buffer, rows being at least two pixels wide -- melf_ctx_create refuses
// a one-pixel-wide template).  Per row: one 64-bit add, the load, one shift.
struct PxColumn {
    const uint8_t* first;  // col - 1, or col in the lane at the buffer's start
    uint32_t shift;        // 8, or 0 there
};
__device__ __forceinline__ PxColumn px_column(const uint8_t* col, const uint8_t* buffer_start)
{
    const bool at_start = col == buffer_start;
    return PxColumn{at_start ? col : col - 1, at_start ? 0u : 8u};
}
__device__ __forceinline__ uint32_t load_px3_row(const PxColumn& c, size_t row_off)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+s"(row_off));  // the offset stays a scalar product: otherwise the compiler folds it into one 64-bit vector multiply-add per row
#endif
    uint32_t v;
    __builtin_memcpy(&v, c.first + row_off, 4);
    return v >> c.shift;
}
// One pixel of the frame: three bytes through load_px3, four as one aligned dword (the 4th byte is never looked at).
template <int PB>
__device__ __forceinline__ uint32_t load_px(const uint8_t* p, const uint8_t* buffer_start)
{
    if constexpr (PB == 4) return *(const uint32_t*)p;
    else return load_px3(p, buffer_start);
}
template <int PB>
__device__ __forceinline__ PxColumn px_column_of(const uint8_t* col, const uint8_t* buffer_start)
{
    if constexpr (PB == 4) return PxColumn{col, 0u};   // aligned 4-byte pixels: the dword is the pixel
    else return px_column(col, buffer_start);
}

// Dial sources.  One is built per wave, `const Src S(src, sargs, P, frame, mx, my)`: src the kernel's DialsSrc, frame the
// workgroup's frame, (mx, my) the match position.  Every pixel leaves a source as a B G R dword (B in byte 0), so that hls_pixel
// and the prefilter see what they see for a BGR frame: the records are those of the BGR frame made from the caller's.  A source has
//   FROM_HLS   packed HLS dials crops (melf_read_dials) instead of camera frames;
//   PB         what a window row unpacks to: 4 = one B G R dword per pixel, 3 = the lane's 12 bytes in three dwords;
//   sb(), bgr(px)   the runtime channel order: the selector offset of the prefilter's byte permutes, a pixel dword to B G R;
//   rstride    bytes between the rows that px() addresses;
//   px(X, Y)   pixel (X, Y) of the dials crop: the 5x5 colour core;
//   column(X), col_px(col, Y, rs_u)   the same for one lane's column X at wave-uniform rows (the exact path);
//   window(wx0, npiece, pc, th1, rs_u, tw)   the lane's share of the window fetch, four pixels a row from window column 4 pc on:
//       .quads          wave-uniform: every 4-pixel piece of the window lies inside the crop's rows and every load inside what
//                       the caller made readable; otherwise nothing is requested and every pixel takes the exact path;
//       .request(g, Y)  the lane's loads for crop row Y, its g-th: what goes into raw[g];
//       .unpack(g, r)   raw[g] -> four B G R dwords (PB 4) or the 12 bytes (PB 3), where the prefilter picks them up.
//   EVEN_QUADS  the lanes' quads must start at an even pixel of the frame (16-bit YUV: see DialYuv16).  The body then asks
//       quad_shift(wx0), 0 or 1 and wave-uniform, starts the quads that many columns left of the window (window(wx0 - shift, ..) with
//       npiece = (ws + shift + 3) / 4) and takes the lane's pixel j for window column 4 pc + j - shift.  False everywhere else, where
//       the body is what it was.
// th1 = P.th - 1 and rs_u = rstride, both made wave-uniform by the body.

// Packed 3- and 4-byte pixels (PB; 4: base, rows and frames 4-byte aligned, the 4th byte ignored): k_dials (B G R, compile-time
// byte selectors; FROM_HLS: packed HLS crops, no window fetch) and k_needles (RT_ORDER: the channel order is the runtime selector
// bsel, 0: B G R, 0x00020002: R G B, and every pixel leaves its load through a byte permute into B G R order).
// The window, round 5: a lane fetches FOUR pixels of a row as one aligned 16-byte load (the 12 bytes and what the alignment adds;
// 4-byte pixels: exactly the four, nothing beyond them), sixteen lanes a row, four rows per instruction -- NR / 4 loads per wave
// instead of NR.  Until then a lane fetched its column's pixel of every row as an unaligned dword: the texture addresser took 12
// cycles per such instruction, and the 784 of a CU's sixteen waves were issued over the launch's first 4.6 us with nothing else to
// do (tools/dials_clock.py: "pixels requested" 9 700 cycles; 4 200 for a wave alone on its SIMD).
template <int PB_, bool RT_ORDER, bool FROM_HLS_ = false>
struct DialPacked {
    static constexpr int PB = PB_;
    static constexpr bool FROM_HLS = FROM_HLS_;
    static constexpr bool EVEN_QUADS = false;
    struct Args { uint32_t bsel; };
    const DialsSrc& src;
    const uint32_t bsel, csel;   // csel: pixel -> B G R in bytes 0..2
    const size_t rstride;
    const uint8_t* const origin;
    __device__ __forceinline__ DialPacked(const DialsSrc& s, const Args& a, const melf_params& P, const uint8_t* frame, int mx, int my)
        : src(s), bsel(a.bsel), csel(a.bsel ? 0x0c000102u : 0x0c020100u), rstride(FROM_HLS ? (size_t)P.tw * 3 : (size_t)s.row_stride),
          origin(FROM_HLS ? frame : frame + (size_t)(s.y0 + my) * s.row_stride + (size_t)(s.x0 + mx) * PB) {}
    __device__ __forceinline__ int quad_shift(int) const { return 0; }
    __device__ __forceinline__ uint32_t sb() const { return RT_ORDER ? bsel : 0u; }
    __device__ __forceinline__ uint32_t bgr(uint32_t px) const
    {
        if constexpr (RT_ORDER) return __builtin_amdgcn_perm(0u, px, csel);
        else return px;
    }
    __device__ __forceinline__ uint32_t px(int X, int Y) const { return bgr(load_px<PB>(origin + (size_t)Y * rstride + (size_t)X * PB, src.base)); }
    __device__ __forceinline__ PxColumn column(int X) const { return px_column_of<PB>(origin + (size_t)X * PB, src.base); }
    __device__ __forceinline__ uint32_t col_px(const PxColumn& c, int Y, int rs_u) const { return bgr(load_px3_row(c, (size_t)((int64_t)Y * rs_u))); }
    struct Window {
        bool quads;
        const uint8_t* lane0;
        int rs_u;
        uint32_t mshift;   // bytes between a load's aligned address and its first pixel (0..3), two bits per load
        __device__ __forceinline__ u32x4v request(int g, int Y)
        {
            const uint8_t* const a = lane0 + (size_t)Y * (size_t)rs_u;
            if constexpr (PB == 4) {
                return load16(a);
            } else {
                mshift |= ((uint32_t)(uintptr_t)a & 3u) << (2 * g);
                return load16((const void*)((uintptr_t)a & ~(uintptr_t)3));
            }
        }
        // 3-byte pixels: the lane's 12 bytes  B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
        __device__ __forceinline__ u32x4v unpack(int g, const u32x4v r) const
        {
            if constexpr (PB == 4) {
                return r;
            } else {
                const uint32_t ms = (mshift >> (2 * g)) & 3u;
                return u32x4v{__builtin_amdgcn_alignbyte(r.y, r.x, ms), __builtin_amdgcn_alignbyte(r.z, r.y, ms), __builtin_amdgcn_alignbyte(r.w, r.z, ms), 0u};
            }
        }
    };
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int th1, int rs_u, int tw) const
    {
        const uint8_t* const buf_end = src.base + src.readable;   // (not frames x stride: the last frame of a padded-stride buffer may end earlier)
        const bool quads = !FROM_HLS && ((uintptr_t)src.base & 3) == 0 && wx0 >= 0 && wx0 + 4 * npiece <= tw &&
                           origin + (size_t)th1 * rstride + (size_t)(wx0 + 4 * npiece) * PB + (PB == 4 ? 0 : 4) <= buf_end;
        return Window{quads, origin + (ptrdiff_t)(wx0 + 4 * min(pc, npiece - 1)) * PB, rs_u, 0u};   // (signed: wx0 may be -1; unused then)
    }
};

// What the other sources share: camera frames that unpack to one B G R dword per pixel in a fixed order, pixels addressed from the
// match position in the frame; the exact path's column pixel is px() again.
template <class Self>
struct DialFrame {
    static constexpr int PB = 4;
    static constexpr bool FROM_HLS = false;
    static constexpr bool EVEN_QUADS = false;
    const DialsSrc& src;
    const uint8_t* const frame;
    const size_t rstride;
    const int fx_m, fy_m;   // the match position in the frame
    __device__ __forceinline__ DialFrame(const DialsSrc& s, const uint8_t* frame_, int mx, int my)
        : src(s), frame(frame_), rstride((size_t)s.row_stride), fx_m(s.x0 + mx), fy_m(s.y0 + my) {}
    __device__ __forceinline__ int quad_shift(int) const { return 0; }
    __device__ __forceinline__ uint32_t sb() const { return 0u; }
    __device__ __forceinline__ uint32_t bgr(uint32_t px) const { return px; }
    __device__ __forceinline__ int column(int X) const { return X; }
    __device__ __forceinline__ uint32_t col_px(int X, int Y, int) const { return static_cast<const Self*>(this)->px(X, Y); }
    // wave-uniform: every piece lies inside the crop's rows (no column clamping: a lane's four pixels stay four neighbours)
    __device__ __forceinline__ static bool pieces_inside(int wx0, int npiece, int tw) { return wx0 >= 0 && wx0 + 4 * npiece <= tw; }
    __device__ __forceinline__ int lane_fx0(int wx0, int npiece, int pc) const { return fx_m + wx0 + 4 * min(pc, npiece - 1); }   // the lane's first pixel in the frame
};

// Four pixels whose Y are the bytes of yd, on the consecutive chroma pairs c0 c1 c2 from the first pixel's on (the lane's first pixel
// odd in the frame: fodd): pixel j sits on pair (j + fodd) >> 1.
__device__ __forceinline__ u32x4v yuv_bgr_on_pairs(uint32_t yd, const YuvChroma& c0, const YuvChroma& c1, const YuvChroma& c2, bool fodd,
                                                   const YuvMatrix& ymat)
{
    return u32x4v{yuv_bgr(yd & 255, c0, ymat), yuv_bgr((yd >> 8) & 255, fodd ? c1 : c0, ymat), yuv_bgr((yd >> 16) & 255, c1, ymat),
                  yuv_bgr(yd >> 24, fodd ? c2 : c1, ymat)};
}

// Planar / semi-planar YUV frames of any subsampling (k_yp_needle, melf_process_yuv_planar*): src the Y plane, `yuv` the chroma
// (YuvPlanarPlanes), any byte alignment; SUBX (0, 1) and CSTEP (1, 2) are compile-time: the four forms of the chroma fetch; sub_y
// is the scalar shift of the chroma row.  Every load fetches Y and the chroma under it and leaves as a B G R dword (melf_device.h:
// yuv_bgr, under the launch's matrix ymat): the core pixel and the exact path's column pixel by three byte loads, a lane's four
// window pixels as one Y dword (inside its row: the pieces lie inside the crop) and the chroma under it, at any parity of the origin.
// SUBX 1: the pairs (fx0 >> 1) .. (fx0 + 3) >> 1, two or three of them, in a load of four samples that starts at the first or, near
// the crop's right edge, as far left of it as keeps the load inside the chroma row of the crop (xlim: the crop's right edge, rounded
// up to a whole pair); the shift is undone
// in unpack.  SUBX 0: the four samples of the four pixels, inside the crop like the Y dword.  CSTEP 1: one unaligned dword of each
// plane; CSTEP 2: one 8-byte load of interleaved pairs from the lower of the two offsets, split by two v_perm_b32 whose selectors
// the order of a pair's bytes exchanges.  Nothing is read outside the crop's rows of the planes.
template <int SUBX, int CSTEP>
struct DialYuvPlanar : DialFrame<DialYuvPlanar<SUBX, CSTEP>> {
    using Base = DialFrame<DialYuvPlanar<SUBX, CSTEP>>;
    struct Args { const YuvPlanarPlanes& yuv; const YuvMatrix& ymat; };
    const YuvMatrix& ymat;
    const int cp_u;
    const uint32_t sy_u;
    const uint8_t *const uplane, *const vplane;
    const bool vfirst;   // CSTEP 2: V before U in a pair (wave-uniform)
    __device__ __forceinline__ DialYuvPlanar(const DialsSrc& s, const uint8_t* frame_, int mx, int my, const YuvMatrix& ymat_, int64_t u_off, int64_t v_off,
                                             int c_pitch, int sub_y, bool vfirst_)
        : Base(s, frame_, mx, my), ymat(ymat_), cp_u(__builtin_amdgcn_readfirstlane(c_pitch)), sy_u((uint32_t)__builtin_amdgcn_readfirstlane(sub_y)),
          uplane(frame_ + (size_t)u_off), vplane(frame_ + (size_t)v_off), vfirst(vfirst_) {}
    __device__ __forceinline__ DialYuvPlanar(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : DialYuvPlanar(s, frame_, mx, my, a.ymat, a.yuv.u_off, a.yuv.v_off, a.yuv.c_pitch, a.yuv.sub_y, a.yuv.v_off < a.yuv.u_off) {}
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        const int fx = this->fx_m + X, fy = this->fy_m + Y;
        const size_t co = (size_t)(fy >> sy_u) * (size_t)cp_u + (size_t)((fx >> SUBX) * CSTEP);
        const int yv = this->frame[(size_t)fy * this->rstride + (size_t)fx];
        return yuv_bgr(yv, yuv_chroma<false>(uplane[co], vplane[co], ymat), ymat);
    }
    struct Window {
        const DialYuvPlanar& S;
        bool quads;
        int rs_u, fx0, cstart;   // the lane's first pixel in the frame; first chroma sample loaded
        uint32_t cshift;         // bits to the lane's first sample
        bool fodd;
        const uint8_t* cplane;   // CSTEP 2: the interleaved plane
        uint32_t usel, vsel;
        __device__ __forceinline__ u32x4v request(int, int Y) const   // {Y dword, chroma, chroma, -}
        {
            const int fy = S.fy_m + Y;
            uint32_t yd;
            __builtin_memcpy(&yd, S.frame + (size_t)fy * (size_t)rs_u + (size_t)fx0, 4);
            const size_t co = (size_t)(fy >> S.sy_u) * (size_t)S.cp_u + (size_t)(cstart * CSTEP);
            if constexpr (CSTEP == 1) {
                uint32_t ud, vd;
                __builtin_memcpy(&ud, S.uplane + co, 4);
                __builtin_memcpy(&vd, S.vplane + co, 4);
                return u32x4v{yd, ud, vd, 0u};
            } else {
                uint32_t cd[2];
                __builtin_memcpy(cd, cplane + co, 8);
                return u32x4v{yd, cd[0], cd[1], 0u};
            }
        }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            uint32_t cu, cv;   // U / V of the samples in bytes 0 ..
            if constexpr (CSTEP == 1) {
                cu = r.y >> cshift; cv = r.z >> cshift;
            } else {
                const uint64_t c = (((uint64_t)r.z << 32) | r.y) >> cshift;   // the pairs from the lane's first on
                const uint32_t lo = (uint32_t)c, hi = (uint32_t)(c >> 32);
                cu = __builtin_amdgcn_perm(hi, lo, usel); cv = __builtin_amdgcn_perm(hi, lo, vsel);
            }
            const YuvChroma c0 = yuv_chroma<false>(cu & 255, cv & 255, S.ymat), c1 = yuv_chroma<false>((cu >> 8) & 255, (cv >> 8) & 255, S.ymat),
                            c2 = yuv_chroma<false>((cu >> 16) & 255, (cv >> 16) & 255, S.ymat);
            if constexpr (SUBX) {
                return yuv_bgr_on_pairs(r.x, c0, c1, c2, fodd, S.ymat);
            } else {   // a sample per pixel
                const YuvChroma c3 = yuv_chroma<false>(cu >> 24, cv >> 24, S.ymat);
                return u32x4v{yuv_bgr(r.x & 255, c0, S.ymat), yuv_bgr((r.x >> 8) & 255, c1, S.ymat), yuv_bgr((r.x >> 16) & 255, c2, S.ymat),
                              yuv_bgr(r.x >> 24, c3, S.ymat)};
            }
        }
    };
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        const int xlim = (this->src.x0 + this->src.crop_cols + 1) & ~1;
        const bool quads = Base::pieces_inside(wx0, npiece, tw) && (SUBX == 0 || xlim >= 8);
        const int fx0 = this->lane_fx0(wx0, npiece, pc);
        const int cstart = SUBX ? min(fx0 >> 1, (xlim >> 1) - 4) : fx0;
        const uint32_t cshift = SUBX ? (uint32_t)((fx0 >> 1) - cstart) * 8u * CSTEP : 0u;
        return Window{*this, quads, rs_u, fx0, cstart, cshift, (bool)(fx0 & 1), vfirst ? vplane : uplane,
                      vfirst ? 0x07050301u : 0x06040200u, vfirst ? 0x06040200u : 0x07050301u};
    }
};

// Planar / semi-planar YUV frames of 16-bit samples (k_y16_needle, melf_process_yuv16*): src the Y plane (strides in bytes), `yuv` the
// chroma and the reduction (Yuv16Planes), everything 2-byte aligned; CSTEP (1, 2, in samples) is compile-time, sub_y, shift and the
// order of a pair's samples wave-uniform values.  A sibling of DialYuvPlanar, not a parameter of it: the samples' size changes every
// load and the window's geometry.  Every sample is reduced to 8 bits where it is unpacked (y16::reduce, or the same as a packed
// 16-bit shift and minimum on two samples), and leaves as the B G R dword the 8-bit source makes of the reduced samples.
// The window: four Y samples are 8 bytes, and the body hands over 16 bytes per lane and row.  Two chroma pairs are 8 more (CSTEP 1:
// a dword of each plane; CSTEP 2: 8 interleaved bytes), and two pairs lie under four pixels exactly when the first is EVEN in the
// frame; from an odd pixel the four touch three pairs, 20 bytes.  So the quads always start even (EVEN_QUADS): when the window's
// first column is odd in the frame -- match position + dial geometry + crop origin, wave-uniform -- they start one column to its
// left and the body places the columns one further right.  Both parities run the same code at the same cost: no wave takes the
// exact path for its parity.  The shift costs no load: ws = 2 R + 5 is odd, so the ws + 1 columns from the even pixel on fit the
// (ws + 3) / 4 quads that hold ws.  What it does cost is the exact path for a window that starts at the DIALS crop's first column
// (wx0 == 0) where that column is odd in the frame, (src.x0 + mx) & 1: its quads would start left of the dials crop's columns, as
// for a window that leaves them anyway.  For a dial with wx0 == 0 that is every frame of one match parity, about half under jitter;
// a dial with wx0 >= 1 never pays it.
// All of a quad's samples are samples of the crop's rows (the four pixels lie inside the crop, the two pairs are theirs), so nothing
// is read outside the planes, and no load has to be moved left at the crop's right edge: none reaches past the pixels' own pairs.
template <int CSTEP>
struct DialYuv16 : DialFrame<DialYuv16<CSTEP>> {
    using Base = DialFrame<DialYuv16<CSTEP>>;
    static constexpr bool EVEN_QUADS = true;
    struct Args { const Yuv16Planes& yuv; const YuvMatrix& ymat; };
    const YuvMatrix& ymat;
    const int cp_u, sy_u;
    const uint32_t sh_u;
    const uint8_t *const uplane, *const vplane;
    const bool vfirst;   // CSTEP 2: V before U in a pair (wave-uniform)
    __device__ __forceinline__ DialYuv16(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : Base(s, frame_, mx, my), ymat(a.ymat), cp_u(__builtin_amdgcn_readfirstlane(a.yuv.c_pitch)), sy_u(__builtin_amdgcn_readfirstlane(a.yuv.sub_y)),
          sh_u((uint32_t)__builtin_amdgcn_readfirstlane(a.yuv.shift)), uplane(frame_ + (size_t)a.yuv.u_off), vplane(frame_ + (size_t)a.yuv.v_off),
          vfirst(a.yuv.v_off < a.yuv.u_off) {}
    __device__ __forceinline__ int quad_shift(int wx0) const { return __builtin_amdgcn_readfirstlane(y16::quad_shift(this->fx_m, wx0)); }
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        const int fx = this->fx_m + X, fy = this->fy_m + Y;
        const size_t co = y16::px_c_off(fy, sy_u, (size_t)cp_u, fx, CSTEP);
        const uint32_t yv = *(const uint16_t*)(this->frame + y16::px_y_off(fy, this->rstride, fx));
        const uint32_t u = *(const uint16_t*)(uplane + co), v = *(const uint16_t*)(vplane + co);
        return yuv_bgr((int)y16::reduce(yv, sh_u), yuv_chroma<false>((int)y16::reduce(u, sh_u), (int)y16::reduce(v, sh_u), ymat), ymat);
    }
    // two 16-bit samples of a dword, each reduced to 8 bits in its half
    __device__ __forceinline__ uint32_t reduce2(uint32_t d) const
    {
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        const u16x2 s2 = {(unsigned short)sh_u, (unsigned short)sh_u}, top = {255, 255};
        return __builtin_bit_cast(uint32_t, __builtin_elementwise_min((u16x2)(__builtin_bit_cast(u16x2, d) >> s2), top));
    }
    struct Window {
        const DialYuv16& S;
        bool quads;
        int rs_u, fx0;           // the lane's first pixel in the frame (even)
        const uint8_t* cplane;   // CSTEP 2: the interleaved plane
        __device__ __forceinline__ u32x4v request(int, int Y) const   // {Y0 Y1, Y2 Y3, chroma, chroma}
        {
            const int fy = S.fy_m + Y;
            uint32_t yd[2];
            __builtin_memcpy(yd, S.frame + y16::dial_y_off(fy, (size_t)rs_u, fx0), y16::DIAL_Y_BYTES);
            const size_t co = y16::dial_c_off(fy, S.sy_u, (size_t)S.cp_u, fx0, CSTEP);
            if constexpr (CSTEP == 1) {
                uint32_t ud, vd;
                __builtin_memcpy(&ud, S.uplane + co, 4);
                __builtin_memcpy(&vd, S.vplane + co, 4);
                return u32x4v{yd[0], yd[1], ud, vd};
            } else {
                uint32_t cd[2];
                __builtin_memcpy(cd, cplane + co, 8);
                return u32x4v{yd[0], yd[1], cd[0], cd[1]};
            }
        }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            const uint32_t y01 = S.reduce2(r.x), y23 = S.reduce2(r.y), ca = S.reduce2(r.z), cb = S.reduce2(r.w);
            uint32_t u0, v0, u1, v1;   // the chroma of pixels 0, 1 and of pixels 2, 3
            if constexpr (CSTEP == 1) {   // ca: U of the two pairs, cb: V
                u0 = ca & 255u; u1 = ca >> 16; v0 = cb & 255u; v1 = cb >> 16;
            } else {                      // ca: the first pair, cb: the second
                const uint32_t f0 = ca & 255u, s0 = ca >> 16, f1 = cb & 255u, s1 = cb >> 16;
                u0 = S.vfirst ? s0 : f0; v0 = S.vfirst ? f0 : s0; u1 = S.vfirst ? s1 : f1; v1 = S.vfirst ? f1 : s1;
            }
            const YuvChroma c0 = yuv_chroma<false>((int)u0, (int)v0, S.ymat), c1 = yuv_chroma<false>((int)u1, (int)v1, S.ymat);
            return u32x4v{yuv_bgr((int)(y01 & 255u), c0, S.ymat), yuv_bgr((int)(y01 >> 16), c0, S.ymat), yuv_bgr((int)(y23 & 255u), c1, S.ymat),
                          yuv_bgr((int)(y23 >> 16), c1, S.ymat)};
        }
    };
    // wx0: the quads' first column (the window's, less quad_shift), npiece: their count
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        return Window{*this, y16::quads_inside(wx0, npiece, tw), rs_u, y16::lane_fx0(this->fx_m, wx0, npiece, pc), vfirst ? vplane : uplane};
    }
};

// NV12 (PLANAR false) / I420 (PLANAR true) frames (k_yneedle): src the Y plane, `yuv` the chroma planes (YuvPlanes).  The 4:2:0
// form of the source above, U before V: the same text, the kernels and their arguments stay their own.
template <bool PLANAR>
struct DialYuv420 : DialYuvPlanar<1, PLANAR ? 1 : 2> {
    struct Args { const YuvPlanes& yuv; const YuvMatrix& ymat; };
    __device__ __forceinline__ DialYuv420(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : DialYuvPlanar<1, PLANAR ? 1 : 2>(s, frame_, mx, my, a.ymat, a.yuv.u_off, a.yuv.v_off, a.yuv.c_pitch, 1, false) {}
};

// Packed YUV 4:2:2 frames (k_p422_needle, melf_process_yuv422*): two pixels per aligned macropixel dword, its byte order the runtime
// permute selector psel (-> Y0 U Y1 V).  One pixel: its macropixel, one aligned dword load.  A lane's four window pixels lie in the
// macropixels (fx0 >> 1) .. (fx0 + 3) >> 1, two of them (fx0 even) or three (odd).  Three aligned dwords per lane and row, from the
// first macropixel or, at the crop's right edge, from one further left, so that the third stays inside the row (mlim: the macropixels
// up to the crop's right edge; the frame's width is even, so the row holds them all).  Only an even fx0 can be moved (its third
// dword is the spare one); the move is undone in unpack.
struct DialP422 : DialFrame<DialP422> {
    struct Args { uint32_t psel; const YuvMatrix& ymat; };
    const uint32_t psel;
    const YuvMatrix& ymat;
    __device__ __forceinline__ DialP422(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : DialFrame(s, frame_, mx, my), psel(a.psel), ymat(a.ymat) {}
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        const int fx = fx_m + X, fy = fy_m + Y;
        const uint32_t c = __builtin_amdgcn_perm(0u, *(const uint32_t*)(frame + (size_t)fy * rstride + (size_t)(fx >> 1) * 4), psel);
        return yuv_bgr((int)((fx & 1 ? c >> 16 : c) & 255u), yuv_chroma<false>((int)((c >> 8) & 255u), (int)(c >> 24), ymat), ymat);
    }
    struct Window {
        const DialP422& S;
        bool quads;
        int rs_u, mstart;   // first macropixel loaded
        bool mshifted, fodd;
        __device__ __forceinline__ u32x4v request(int, int Y) const
        {
            const int fy = S.fy_m + Y;
            uint32_t md[3];
            __builtin_memcpy(md, (const uint32_t*)(S.frame + (size_t)fy * (size_t)rs_u) + mstart, 12);
            return u32x4v{md[0], md[1], md[2], 0u};
        }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            const uint32_t ma = __builtin_amdgcn_perm(0u, mshifted ? r.y : r.x, S.psel), mb = __builtin_amdgcn_perm(0u, mshifted ? r.z : r.y, S.psel),
                           mc = __builtin_amdgcn_perm(0u, r.z, S.psel);   // Y0 U Y1 V each
            const YuvChroma c0 = yuv_chroma<false>((int)((ma >> 8) & 255u), (int)(ma >> 24), S.ymat), c1 = yuv_chroma<false>((int)((mb >> 8) & 255u), (int)(mb >> 24), S.ymat),
                            c2 = yuv_chroma<false>((int)((mc >> 8) & 255u), (int)(mc >> 24), S.ymat);
            const uint32_t y4 = __builtin_amdgcn_perm(mb, ma, 0x06040200u);                  // Y of the pixels of ma, mb
            const uint32_t yd = fodd ? __builtin_amdgcn_perm(mc, y4, 0x04030201u) : y4;      // Y of the lane's four
            return yuv_bgr_on_pairs(yd, c0, c1, c2, fodd, S.ymat);
        }
    };
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        const int mlim = (src.x0 + src.crop_cols + 1) >> 1;
        const bool quads = pieces_inside(wx0, npiece, tw) && mlim >= 3;
        const int fx0 = lane_fx0(wx0, npiece, pc);
        const int mstart = min(fx0 >> 1, mlim - 3);
        return Window{*this, quads, rs_u, mstart, (fx0 >> 1) != mstart, (bool)(fx0 & 1)};
    }
};

// Packed 10-bit YUV 4:2:2 frames (melf_process_yuv422_10*), both formats: every sample leaves its load as its top 8 bits, and from
// Y0 U Y1 V on the arithmetic is DialP422's.  The quads start at an even pixel of the frame (EVEN_QUADS, as DialYuv16): four pixels
// from an even one are two whole pairs, 16 bytes in either format.  Offsets and guards: melf_p10_addr.h.
// What a pair's four samples make: two B G R dwords.
__device__ __forceinline__ void p10_pair_bgr(uint32_t y0, uint32_t u, uint32_t y1, uint32_t v, const YuvMatrix& ymat, uint32_t& b0, uint32_t& b1)
{
    const YuvChroma c = yuv_chroma<false>((int)u, (int)v, ymat);
    b0 = yuv_bgr((int)y0, c, ymat);
    b1 = yuv_bgr((int)y1, c, ymat);
}

// v210 (k_v210_needle): rows of whole 16-byte groups, six pixels each, twelve 10-bit fields U Y V Y ...  One pixel: the two words
// of its group that hold its three fields.  A lane's quad from the even pixel fx0, p = fx0 % 6: the aligned group (p 0, 2) or the
// 16 bytes from its third word on (p 4), one load16; the twelve fields of the 16 bytes are extracted at fixed positions and the
// quad's eight picked by p -- which differs from lane to lane -- with selects, so every register array is indexed by constants.
struct DialV210 : DialFrame<DialV210> {
    static constexpr bool EVEN_QUADS = true;
    struct Args { const YuvMatrix& ymat; };
    const YuvMatrix& ymat;
    __device__ __forceinline__ DialV210(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : DialFrame(s, frame_, mx, my), ymat(a.ymat) {}
    __device__ __forceinline__ int quad_shift(int wx0) const { return __builtin_amdgcn_readfirstlane(p10::quad_shift(fx_m, wx0)); }
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        const int fx = fx_m + X, fy = fy_m + Y;
        const uint32_t* w = (const uint32_t*)(frame + p10::v210_px_off(fy, rstride, fx));
        const int ph = p10::v210_phase(fx);
        const uint32_t s = p10::v210_px_yuv(w[0], w[1], ph >> 1, ph & 1);
        return yuv_bgr((int)(s & 255u), yuv_chroma<false>((int)((s >> 8) & 255u), (int)(s >> 16), ymat), ymat);
    }
    struct Window {
        const DialV210& S;
        bool quads;
        int rs_u, fx0;   // the lane's first pixel in the frame (even)
        int f0;          // the quad's first field among the twelve of the 16 bytes loaded: 0, 4 or 2
        __device__ __forceinline__ u32x4v request(int, int Y) const { return load16(S.frame + p10::v210_dial_off(S.fy_m + Y, (size_t)rs_u, fx0)); }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            uint32_t F[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) F[i] = p10::field8(r[p10::field_word(i)], p10::field_bit(i));
            uint32_t q[8];   // U Y V Y U Y V Y of the quad
#pragma unroll
            for (int k = 0; k < 8; ++k) q[k] = f0 == 0 ? F[k] : (f0 == 4 ? F[k + 4] : F[k + 2]);
            u32x4v o;
            uint32_t b0, b1;
            p10_pair_bgr(q[1], q[0], q[3], q[2], S.ymat, b0, b1);
            o.x = b0; o.y = b1;
            p10_pair_bgr(q[5], q[4], q[7], q[6], S.ymat, b0, b1);
            o.z = b0; o.w = b1;
            return o;
        }
    };
    // wx0: the quads' first column (the window's, less quad_shift), npiece: their count
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        const int fx0 = p10::lane_fx0(fx_m, wx0, npiece, pc);
        return Window{*this, p10::quads_inside(wx0, npiece, tw), rs_u, fx0, p10::v210_dial_field0(p10::v210_phase(fx0))};
    }
};

// Y210 / Y212 / Y216 (k_y210_needle): macropixels of four MSB-aligned 16-bit words Y0 U Y1 V.  One pixel: its macropixel, two
// aligned dwords.  A lane's quad from an even pixel is two macropixels, one 16-byte load, 8-byte aligned; a byte permute per
// macropixel picks the four high bytes.
struct DialY210 : DialFrame<DialY210> {
    static constexpr bool EVEN_QUADS = true;
    struct Args { const YuvMatrix& ymat; };
    const YuvMatrix& ymat;
    __device__ __forceinline__ DialY210(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : DialFrame(s, frame_, mx, my), ymat(a.ymat) {}
    __device__ __forceinline__ int quad_shift(int wx0) const { return __builtin_amdgcn_readfirstlane(p10::quad_shift(fx_m, wx0)); }
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        const int fx = fx_m + X, fy = fy_m + Y;
        const uint32_t* w = (const uint32_t*)(frame + p10::y210_px_off(fy, rstride, fx));
        const uint32_t s = p10::y210_px_yuv(w[0], w[1], fx & 1);
        return yuv_bgr((int)(s & 255u), yuv_chroma<false>((int)((s >> 8) & 255u), (int)(s >> 16), ymat), ymat);
    }
    struct Window {
        const DialY210& S;
        bool quads;
        int rs_u, fx0;   // the lane's first pixel in the frame (even)
        __device__ __forceinline__ u32x4v request(int, int Y) const { return load16(S.frame + p10::y210_dial_off(S.fy_m + Y, (size_t)rs_u, fx0)); }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            const uint32_t ma = __builtin_amdgcn_perm(r.y, r.x, 0x07050301u), mb = __builtin_amdgcn_perm(r.w, r.z, 0x07050301u);   // Y0 U Y1 V each
            u32x4v o;
            uint32_t b0, b1;
            p10_pair_bgr(ma & 255u, (ma >> 8) & 255u, (ma >> 16) & 255u, ma >> 24, S.ymat, b0, b1);
            o.x = b0; o.y = b1;
            p10_pair_bgr(mb & 255u, (mb >> 8) & 255u, (mb >> 16) & 255u, mb >> 24, S.ymat, b0, b1);
            o.z = b0; o.w = b1;
            return o;
        }
    };
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        return Window{*this, p10::quads_inside(wx0, npiece, tw), rs_u, p10::lane_fx0(fx_m, wx0, npiece, pc)};
    }
};

// 32-bit packed 4:4:4 frames (k_p32_needle, melf_process_packed32*): one little-endian word per pixel, base, rows and frames 4-byte
// aligned; three 8-bit reads at the positions of `fields` (Packed32Fields, the same for every lane: scalar operands), YUV: Y, U, V
// under the launch's matrix, else R, G, B.  One pixel: its word, one aligned dword.  A lane's four window pixels are their four
// words, one 16-byte load from a 4-byte aligned address exactly as DialPacked<4>'s -- the four are pixels of the crop's rows when the
// pieces lie inside the crop, so nothing is read outside a row, and no quad has to start at an even pixel.  unpack: three v_bfe_u32
// per pixel, then yuv_chroma / yuv_bgr with one chroma per pixel as DialYuvPlanar<0, 1> (YUV), or two v_lshl_or_b32 into B G R.
template <bool YUV>
struct DialWord32 : DialFrame<DialWord32<YUV>> {
    using Base = DialFrame<DialWord32<YUV>>;
    struct Args { const Packed32Fields& fields; const YuvMatrix& ymat; };
    const Packed32Fields& fields;
    const YuvMatrix& ymat;   // (YUV only)
    __device__ __forceinline__ DialWord32(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : Base(s, frame_, mx, my), fields(a.fields), ymat(a.ymat) {}
    // a word -> the B G R dword
    __device__ __forceinline__ uint32_t word_bgr(uint32_t w) const
    {
        if constexpr (YUV)
            return yuv_bgr((int)p32::read8(w, fields.pos[0]), yuv_chroma<false>((int)p32::read8(w, fields.pos[1]), (int)p32::read8(w, fields.pos[2]), ymat), ymat);
        else
            return p32::rgb_bgr(w, fields);
    }
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        return word_bgr(*(const uint32_t*)(this->frame + p32::px_off(this->fy_m + Y, this->rstride, this->fx_m + X)));
    }
    struct Window {
        const DialWord32& S;
        bool quads;
        int rs_u, fx0;   // the lane's first pixel in the frame
        __device__ __forceinline__ u32x4v request(int, int Y) const { return load16(S.frame + p32::dial_off(S.fy_m + Y, (size_t)rs_u, fx0)); }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            return u32x4v{S.word_bgr(r.x), S.word_bgr(r.y), S.word_bgr(r.z), S.word_bgr(r.w)};
        }
    };
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        return Window{*this, Base::pieces_inside(wx0, npiece, tw), rs_u, this->lane_fx0(wx0, npiece, pc)};
    }
};

// Planar frames (k_planar_needle, melf_process_planes*): the B, G and R planes at `planes` (PlanarPlanes) in a frame, any byte
// alignment.  The core pixel and the exact path's column pixel are three byte loads; a lane's four window pixels are one unaligned
// dword per plane, four consecutive bytes of each plane's row inside the crop (and so inside the frame's row): nothing is read
// outside the planes' samples, whatever the alignment.  unpack turns {B0 B1 B2 B3, G0 G1 G2 G3, R0 R1 R2 R3} into four B G R dwords
// by six v_perm_b32.
struct DialPlanarRgb : DialFrame<DialPlanarRgb> {
    struct Args { const PlanarPlanes& planes; };
    const uint8_t *const bplane, *const gplane, *const rplane;
    __device__ __forceinline__ DialPlanarRgb(const DialsSrc& s, const Args& a, const melf_params&, const uint8_t* frame_, int mx, int my)
        : DialFrame(s, frame_, mx, my), bplane(frame_ + (size_t)a.planes.b_off), gplane(frame_ + (size_t)a.planes.g_off),
          rplane(frame_ + (size_t)a.planes.r_off) {}
    __device__ __forceinline__ uint32_t px(int X, int Y) const
    {
        const size_t o = (size_t)(fy_m + Y) * rstride + (size_t)(fx_m + X);
        return (uint32_t)bplane[o] | (uint32_t)gplane[o] << 8 | (uint32_t)rplane[o] << 16;
    }
    struct Window {
        const DialPlanarRgb& S;
        bool quads;
        int rs_u, fx0;   // the lane's first pixel in the frame
        __device__ __forceinline__ u32x4v request(int, int Y) const
        {
            const int fy = S.fy_m + Y;
            const size_t o = (size_t)fy * (size_t)rs_u + (size_t)fx0;
            uint32_t bd, gd, rd;
            __builtin_memcpy(&bd, S.bplane + o, 4);
            __builtin_memcpy(&gd, S.gplane + o, 4);
            __builtin_memcpy(&rd, S.rplane + o, 4);
            return u32x4v{bd, gd, rd, 0u};
        }
        __device__ __forceinline__ u32x4v unpack(int, const u32x4v r) const
        {
            const uint32_t t01 = __builtin_amdgcn_perm(r.y, r.x, 0x05010400u), t23 = __builtin_amdgcn_perm(r.y, r.x, 0x07030602u);   // B0 G0 B1 G1, B2 G2 B3 G3
            return u32x4v{__builtin_amdgcn_perm(r.z, t01, 0x0c040100u), __builtin_amdgcn_perm(r.z, t01, 0x0c050302u),
                          __builtin_amdgcn_perm(r.z, t23, 0x0c060100u), __builtin_amdgcn_perm(r.z, t23, 0x0c070302u)};
        }
    };
    __device__ __forceinline__ Window window(int wx0, int npiece, int pc, int, int rs_u, int tw) const
    {
        return Window{*this, pieces_inside(wx0, npiece, tw), rs_u, lane_fx0(wx0, npiece, pc)};
    }
};

}  // namespace melf
