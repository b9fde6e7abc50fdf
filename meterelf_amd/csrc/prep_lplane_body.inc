// The body of k_prep_lplane and k_lplane_px4 (k_match_mfma.hip), included by both kernels: everything but the pixel loads is
// shared, and each kernel compiles to what one kernel body gives (a force-inlined function shared by them changed the register
// allocation of the existing instantiations).  In scope: the kernel's arguments and
//   PX  1 = packed single-channel u8 images, 3 = 3-byte pixels (BGR / RGB: L = (max + min) / 2 does not depend on the channel
//       order), 4 = 4-byte pixels (BGRA / RGBA, base, rows and frames 4-byte aligned, the 4th byte ignored): 32 pixels are 128
//       bytes, eight aligned 16-byte loads, no gather.
//   With MELF_YUV_BODY defined by the including kernel (k_lplane_yuv): PX 20 = NV12, 21 = I420 frames, the chroma planes in `yuv`
//       (YuvPlanes); src describes the Y plane.  A lane's window starts at the EVEN pixel at or left of its first one: 34 Y bytes and
//       the 17 chroma pairs under them (NV12 34 interleaved bytes, I420 17 + 17), as aligned dwords; an odd crop origin costs the
//       one pixel of overlap (the 34 results are shifted by a byte at the end), not a second code path.
//   With MELF_P422_BODY defined instead (k_p422_lplane): PX 22 = packed YUV 4:2:2 frames, two pixels per aligned 4-byte macropixel,
//       its byte order the runtime permute selector psel (-> Y0 U Y1 V).  The same even-pixel window is 17 consecutive aligned
//       dwords, each with both Y samples and the chroma pair: no gather, no chroma loads; the odd origin as above.
//   With MELF_PLANAR_BODY defined instead (k_planar_lplane): PX 23 = planar frames (melf_process_planes*), the B, G and R planes at
//       `planes` (PlanarPlanes) in a frame, any byte alignment.  A lane's 32 pixels are 32 consecutive bytes of each plane: nine
//       aligned dwords per plane, shifted by v_alignbit at that plane's own byte phase (the three phases differ when offsets and
//       pitch are arbitrary).  The aligned window reaches up to 3 bytes to the left of the lane's first sample and up to 35 behind it:
//       it must not start before the caller's base nor end behind the buffer, or the lane takes byte loads.
//   With MELF_YUVP_BODY defined instead (k_yp_lplane): PX 24 = planar / semi-planar YUV frames of any subsampling
//       (melf_process_yuv_planar*), the chroma in `yuv` (YuvPlanarPlanes), any byte alignment; SUBX (0, 1) and CSTEP (1, 2) are
//       compile-time: the four forms of the chroma fetch.  The even-pixel window of 34 Y bytes as for PX 20 / 21; the chroma under it
//       is 34 >> SUBX samples: CSTEP 1 that many bytes of each plane, at each plane's own byte phase (load_window, k_match_mfma.hip:
//       aligned dwords and v_alignbit, as for PX 23), CSTEP 2 twice as many interleaved bytes from the lower of the two offsets, one
//       runtime v_perm_b32 per dword putting U before V.  sub_y is the scalar shift of the chroma row.  No window may start before
//       the caller's base nor end behind the buffer, or the lane takes byte loads of the crop's own samples.
//   With MELF_Y16_BODY defined instead (k_y16_lplane): PX 25 = planar / semi-planar YUV frames of 16-bit samples
//       (melf_process_yuv16*), the chroma in `yuv` (Yuv16Planes), everything 2-byte aligned; CSTEP (1, 2, in samples) is compile-time.
//       The even-pixel window is 34 Y samples (68 bytes) and the 17 chroma pairs under them (CSTEP 1: 34 bytes of each plane, CSTEP 2:
//       68 interleaved bytes from the lower of the two offsets): aligned dwords and v_alignbit at the 2-byte phase (load_window16,
//       k_match_mfma.hip), two samples a dword reduced to 8 bits by a packed 16-bit shift and minimum and packed four to a dword --
//       from there on the arm is PX 24's.  Offsets, window lengths, rows_safe and the lane's own test: melf_y16_addr.h.
//   With MELF_V210_BODY defined instead (k_v210_lplane): PX 26 = v210 frames (melf_process_yuv422_10*), rows of whole 16-byte groups
//       of six pixels, everything 16-byte aligned.  The even-pixel window of 34 pixels is 17 pairs from pair slot s = (xs / 2) % 3 of
//       the window's first group, which differs from lane to lane (32 pixels advance the slot by one): up to seven aligned 16-byte
//       loads, of which a lane makes those that hold its own pixels (the rest of the window reads as zero), all 21 pairs of the seven
//       groups unpacked to Y0 U Y1 V at fixed positions and 17 picked by unrolled selects on s: every register array is indexed by
//       constants.  From the 17 dwords on the arm is PX 22's.  No load can leave the crop's row: there is no per-pixel path.
//   With MELF_Y210_BODY defined instead (k_y210_lplane): PX 27 = Y210 / Y212 / Y216 frames, macropixels of four 16-bit words, everything
//       8-byte aligned.  The window is 17 macropixels, 34 aligned dwords as eight 16-byte loads and two dwords; one byte permute per
//       macropixel picks the high bytes Y0 U Y1 V, and from there on the arm is PX 22's.  Offsets, rows_safe and the lane's own
//       test of both arms: melf_p10_addr.h.
//   With MELF_P32_BODY defined instead (k_p32_lplane): PX 28 / 29 = 32-bit packed 4:4:4 frames (melf_process_packed32*), one word per
//       pixel, everything 4-byte aligned, three 8-bit reads at the positions of `fields` (Packed32Fields: scalars).  The loads are
//       PX 4's, taken from the same functions of melf_prep_addr.h: 32 pixels are 128 bytes, eight 16-byte loads, guarded like PX 4's
//       (rows_safe per row, the lane's own test, one dword per pixel where both fail).  PX 28: the reads are Y, U, V, L straight from
//       them (yuv_lightness, one chroma per pixel); PX 29: they are R, G, B, L from the largest and the smallest as for PX 4.
// The 8-bit arms (PX 3, 4, 20 .. 24) compute their windows' offsets and lengths, rows_safe and the lane's own test with the functions
// of melf_prep_addr.h, as PX 25 does with melf_y16_addr.h: tests/prep_bounds_main.cpp sweeps the same functions on the CPU.
    constexpr int PB = prep::packed_pb(PX);     // bytes per pixel of the frame reads
    constexpr int WIN = prep::packed_win(PX);   // bytes a lane's 32-pixel load window spans
    __shared__ __attribute__((aligned(16))) uint32_t tile[8 * 2 * 32 * 4];  // [kb][h][n][16 B], one chunk of 8 blocks
    extern __shared__ int16_t pre_dyn[];                                    // [32][nkb * 32 + 8]: inclusive prefix of L' per frame (mod 2^16)
    const int pstride = nkb * 32 + 8;
    const int y = blockIdx.x, grp = blockIdx.y;
    const int t = threadIdx.x, n = t >> 3, kl = t & 7;
    const int f = grp * 32 + n;
    int carry = 0;  // prefix of the blocks before this chunk (per frame, same in its 8 lanes)
    // (wave-uniform, once) every 100-byte gather window of this row, in every frame of the group, ends inside the caller's buffer -- all
    // rows but the last few of the last frame; the per-lane pointer test below then never runs (as the branch condition of every
    // thread it cost 10 % of the kernel: profiles/r06/prep_bisect.txt)
#ifdef MELF_YUV_BODY
    (void)PB; (void)WIN;
    // (the same for the three windows of a YUV lane: 40 bytes from the Y sample and from the chroma samples of its even pixel)
    const int xodd = src.x0 & 1;
    const size_t yuv_last = (size_t)prep::last_frame(grp, nframes) * src.frame_stride;
    const size_t yuv_crow = prep::yuv420_crow(src.y0 + y, yuv.c_pitch);
    const int yuv_xlast = prep::yuv420_xlast(src.x0, nkb);
    const bool rows_safe = prep::yuv420_rows_safe(yuv_last, src.y0 + y, src.row_stride, yuv_xlast, yuv.u_off, yuv.v_off, yuv_crow, PX == 20, src.readable);
#elif defined(MELF_P422_BODY)
    (void)PB; (void)WIN;
    // (the same for the 68-byte window of a 4:2:2 lane: 17 macropixels from the one of its even pixel)
    const int xodd = src.x0 & 1;
    const bool rows_safe = prep::p422_rows_safe(grp, nframes, src.frame_stride, src.y0 + y, src.row_stride, src.x0, nkb, src.readable);
#elif defined(MELF_YUVP_BODY)
    (void)PB; (void)WIN;
    // (the same for the windows of a lane of these frames: 40 bytes from the Y sample of its even pixel, CB + 3 bytes rounded up to
    // dwords from its first chroma sample in each plane (CSTEP 1) or in the interleaved plane (CSTEP 2) -- and for their first dword:
    // with a base that is not 4-byte aligned the aligned window of the buffer's very first samples would start before it)
    constexpr int NC = prep::yuvp_nc(SUBX);          // chroma samples under a window
    constexpr int CB = prep::yuvp_cb(SUBX, CSTEP);   // bytes of a chroma window
    constexpr int CWIN = prep::yuvp_cwin(SUBX, CSTEP);   // bytes its aligned dwords span
    const int xodd = src.x0 & 1;
    const uint32_t yp_bm = (uint32_t)((size_t)src.base & 3);
    const bool yp_swap = yuv.v_off < yuv.u_off;      // CSTEP 2: V before U in a pair (NV21, NV61, NV42)
    const size_t yp_c0 = (size_t)min(yuv.u_off, yuv.v_off), yp_c1 = (size_t)max(yuv.u_off, yuv.v_off);
    const size_t yp_first = (size_t)grp * 32 * src.frame_stride, yp_last = (size_t)prep::last_frame(grp, nframes) * src.frame_stride;
    const size_t yp_yrow = (size_t)(src.y0 + y) * src.row_stride;
    const size_t yp_crow = (size_t)((src.y0 + y) >> yuv.sub_y) * (size_t)yuv.c_pitch;
    const int yp_x0 = src.x0 & ~1, yp_xlast = yp_x0 + 32 * (nkb - 1);
    const bool rows_safe = prep::yuvp_rows_safe(yp_bm, yp_first, yp_last, yp_yrow, yp_crow, yp_c0, yp_c1, yp_x0, yp_xlast, SUBX, CSTEP, CWIN, src.readable);
#elif defined(MELF_Y16_BODY)
    (void)PB; (void)WIN;
    // (the same for the windows of a lane of these frames, at the buffer's first bytes as well as at its last: y16::prep_rows_safe)
    constexpr int CB = 34 * CSTEP;                   // bytes of a chroma window
    const int xodd = src.x0 & 1;
    const bool yp_swap = yuv.v_off < yuv.u_off;      // CSTEP 2: V before U in a pair
    const uint32_t y16_shift = (uint32_t)yuv.shift;
    const y16::PrepRow prow16 = y16::prep_row((size_t)src.base, src.frame_stride, (size_t)src.row_stride, src.x0, src.y0, y, grp, nframes, nkb,
                                              yuv.u_off, yuv.v_off, (size_t)yuv.c_pitch, yuv.sub_y);
    const bool rows_safe = y16::prep_rows_safe(prow16, CSTEP, src.readable);
#elif defined(MELF_V210_BODY)
    (void)PB; (void)WIN;
    // (here: every live lane of the row holds pixels of the window's first six groups, which then are loaded without a test of
    // the lane's own)
    const int xodd = src.x0 & 1;
    const bool rows_safe = p10::v210_rows_safe(src.x0, src.cols, nkb);
#elif defined(MELF_Y210_BODY)
    (void)PB; (void)WIN;
    // (the same for the 136-byte window of a Y210 lane: 17 macropixels from the one of its even pixel)
    const int xodd = src.x0 & 1;
    const bool rows_safe = p10::y210_rows_safe(grp, nframes, src.frame_stride, src.y0 + y, (size_t)src.row_stride, src.x0, nkb, src.readable);
#elif defined(MELF_P32_BODY)
    (void)PB; (void)WIN;
    // (the same for the 128-byte window of a lane of 4-byte words: PX 4's test)
    const bool rows_safe = prep::packed_rows_safe(grp, nframes, src.frame_stride, src.y0 + y, src.row_stride, src.x0, nkb, prep::packed_pb(4), prep::packed_win(4), src.readable);
#elif defined(MELF_PLANAR_BODY)
    (void)PB; (void)WIN;
    // (the same for the three 36-byte windows of a planar lane, and for their first dword: with a base that is not 4-byte aligned
    // the aligned window of the very first samples of the buffer would start before it)
    const uint32_t pl_bm = (uint32_t)((size_t)src.base & 3);
    const size_t pl_row = prep::planar_row(src.y0 + y, src.row_stride, src.x0);
    const size_t pl_lo = (size_t)min(min(planes.b_off, planes.g_off), planes.r_off), pl_hi = (size_t)max(max(planes.b_off, planes.g_off), planes.r_off);
    const bool rows_safe = prep::planar_rows_safe(pl_bm, grp, nframes, src.frame_stride, pl_lo, pl_hi, pl_row, nkb, src.readable);
#else
    const bool rows_safe = prep::packed_rows_safe(grp, nframes, src.frame_stride, src.y0 + y, src.row_stride, src.x0, nkb, PB, WIN, src.readable);
#endif
    u32x4m* out = (u32x4m*)(Lg + ((size_t)grp * rows_pad + y) * (size_t)nkb * 1024);
    for (int kc = 0; kc < nkb; kc += 8) {
        const int kb = kc + kl;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // 32 output bytes (L' = 0 <=> pad)
        const bool live = kb < nkb && f < nframes && y < src.rows && kb * 32 < src.cols;  // uniform per wave except ragged tails
        if (live) {
            const uint8_t* prow = src.base + (size_t)f * src.frame_stride + (size_t)(src.y0 + y) * src.row_stride;
            const int xbeg = kb * 32;
            const int npx = min(32, src.cols - xbeg);  // < 32 only in the last block: masked below, not branched on
#ifdef MELF_YUV_BODY
            if (PX == 20 || PX == 21) {
                constexpr bool NV12 = PX == 20;
                const int xs = (src.x0 + xbeg) & ~1;   // the window's first pixel (even)
                const size_t fo = (size_t)f * src.frame_stride;
                const size_t yo = prep::yuv420_y_off(fo, src.y0 + y, src.row_stride, xs);
                const size_t uo = prep::yuv420_c_off(fo, yuv.u_off, yuv_crow, xs, NV12);
                const size_t vo = prep::yuv420_c_off(fo, yuv.v_off, yuv_crow, xs, false);   // (I420 only)
                // 10 aligned dwords cover 34 bytes (+ 3 of misalignment), 6 the 17 bytes of an I420 chroma row's share; the windows
                // may reach past the crop (never used: masked) but must stay inside the caller's buffer
                if (rows_safe || prep::yuv420_lane_ok(yo, uo, vo, NV12, src.readable)) {
                    uint32_t ya[9], ua[9], va[5];
                    {
                        const uint8_t* p = src.base + yo;
                        const uint32_t mis = (uint32_t)((size_t)p & 3);
                        const uint32_t* q = (const uint32_t*)(p - mis);
                        uint32_t d[10];
#pragma unroll
                        for (int i = 0; i < 10; ++i) d[i] = q[i];
#pragma unroll
                        for (int i = 0; i < 9; ++i) ya[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], mis * 8u);
                    }
                    if (NV12) {
                        const uint8_t* p = src.base + uo;
                        const uint32_t mis = (uint32_t)((size_t)p & 3);
                        const uint32_t* q = (const uint32_t*)(p - mis);
                        uint32_t d[10];
#pragma unroll
                        for (int i = 0; i < 10; ++i) d[i] = q[i];
#pragma unroll
                        for (int i = 0; i < 9; ++i) ua[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], mis * 8u);
                    } else {
                        const uint8_t* pu = src.base + uo;
                        const uint8_t* pv = src.base + vo;
                        const uint32_t misu = (uint32_t)((size_t)pu & 3), misv = (uint32_t)((size_t)pv & 3);
                        const uint32_t* qu = (const uint32_t*)(pu - misu);
                        const uint32_t* qv = (const uint32_t*)(pv - misv);
                        uint32_t du[6], dv[6];
#pragma unroll
                        for (int i = 0; i < 6; ++i) { du[i] = qu[i]; dv[i] = qv[i]; }
#pragma unroll
                        for (int i = 0; i < 5; ++i) {
                            ua[i] = __builtin_amdgcn_alignbit(du[i + 1], du[i], misu * 8u);
                            va[i] = __builtin_amdgcn_alignbit(dv[i + 1], dv[i], misv * 8u);
                        }
                    }
                    uint32_t wl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // L' of the window's 34 pixels
#pragma unroll
                    for (int j = 0; j < 17; ++j) {
                        int U, V;
                        if (NV12) {
                            U = (int)((ua[j >> 1] >> ((j & 1) * 16)) & 255u);
                            V = (int)((ua[j >> 1] >> ((j & 1) * 16 + 8)) & 255u);
                        } else {
                            U = (int)((ua[j >> 2] >> ((j & 3) * 8)) & 255u);
                            V = (int)((va[j >> 2] >> ((j & 3) * 8)) & 255u);
                        }
                        const YuvChroma c = yuv_chroma(U, V, mx);
                        const int cmax = yuv_cmax(c), cmin = yuv_cmin(c);
#pragma unroll
                        for (int q2 = 0; q2 < 2; ++q2) {
                            const int k = 2 * j + q2;
                            const int L = yuv_lightness((int)((ya[k >> 2] >> ((k & 3) * 8)) & 255u), cmax, cmin, mx);
                            wl[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                        }
                    }
                    // the lane's 32 pixels start at byte xodd of the window
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(wl[i + 1], wl[i], (uint32_t)xodd * 8u);
                } else {  // last bytes of the frame buffer: byte loads
                    const uint8_t* py = src.base + fo + (size_t)(src.y0 + y) * src.row_stride + (size_t)(src.x0 + xbeg);
                    const uint8_t* pu = src.base + fo + (size_t)yuv.u_off + yuv_crow;
                    const uint8_t* pv = src.base + fo + (size_t)yuv.v_off + yuv_crow;
                    for (int k = 0; k < npx; ++k) {
                        const int cx = (src.x0 + xbeg + k) >> 1;
                        const YuvChroma c = yuv_chroma(pu[NV12 ? 2 * cx : cx], pv[NV12 ? 2 * cx : cx], mx);
                        const int L = yuv_lightness(py[k], yuv_cmax(c), yuv_cmin(c), mx);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#elif defined(MELF_P422_BODY)
            if (PX == 22) {
                const int xs = (src.x0 + xbeg) & ~1;   // the window's first pixel (even)
                const size_t o = prep::p422_x_off(xs);
                // the window may reach past the crop and the row (never used: masked) but must stay inside the caller's buffer
                if (rows_safe || prep::p422_lane_ok(f, src.frame_stride, src.y0 + y, src.row_stride, o, src.readable)) {
                    const u32x4a4* q = (const u32x4a4*)(prow + o);
                    u32x4a4 d[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) d[i] = q[i];
                    const uint32_t d16 = ((const uint32_t*)(prow + o))[16];
                    uint32_t wl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // L' of the window's 34 pixels
#pragma unroll
                    for (int j = 0; j < 17; ++j) {
                        const uint32_t m = __builtin_amdgcn_perm(0u, j < 16 ? d[j >> 2][j & 3] : d16, psel);   // Y0 U Y1 V
                        const YuvChroma c = yuv_chroma((int)((m >> 8) & 255u), (int)(m >> 24), mx);
                        const int cmax = yuv_cmax(c), cmin = yuv_cmin(c);
                        const int L0 = yuv_lightness((int)(m & 255u), cmax, cmin, mx), L1 = yuv_lightness((int)((m >> 16) & 255u), cmax, cmin, mx);
                        wl[j >> 1] |= ((uint32_t)((L0 - 128) & 255) | (uint32_t)((L1 - 128) & 255) << 8) << ((j & 1) * 16);
                    }
                    // the lane's 32 pixels start at byte xodd of the window
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(wl[i + 1], wl[i], (uint32_t)xodd * 8u);
                } else {  // last bytes of the frame buffer: one macropixel per pixel, inside the row
                    for (int k = 0; k < npx; ++k) {
                        const int fx = src.x0 + xbeg + k;
                        const uint32_t m = __builtin_amdgcn_perm(0u, ((const uint32_t*)prow)[fx >> 1], psel);
                        const YuvChroma c = yuv_chroma((int)((m >> 8) & 255u), (int)(m >> 24), mx);
                        const int L = yuv_lightness((int)((fx & 1 ? m >> 16 : m) & 255u), yuv_cmax(c), yuv_cmin(c), mx);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#elif defined(MELF_YUVP_BODY)
            if (PX == 24) {
                const int xs = (src.x0 + xbeg) & ~1;   // the window's first pixel (even)
                const size_t fo = (size_t)f * src.frame_stride;
                const size_t yo = fo + yp_yrow + (size_t)xs;
                const size_t cx = prep::yuvp_cx(xs, SUBX, CSTEP);
                const size_t uo = fo + (CSTEP == 2 ? yp_c0 : (size_t)yuv.u_off) + yp_crow + cx;   // CSTEP 2: the interleaved window
                const size_t vo = fo + (size_t)yuv.v_off + yp_crow + cx;                          // (CSTEP 1 only)
                const uint32_t my = (yp_bm + (uint32_t)yo) & 3u, mu = (yp_bm + (uint32_t)uo) & 3u, mv = (yp_bm + (uint32_t)vo) & 3u;
                // the windows may reach past the crop and the row (never used: masked) but must stay inside the caller's buffer, at its
                // first bytes as well as at its last
                if (rows_safe || prep::yuvp_lane_ok(yo, my, uo, mu, vo, mv, CSTEP, CWIN, src.readable)) {
                    uint32_t ya[9], ua[(NC + 3) / 4], va[(NC + 3) / 4];   // Y, U, V of the window, a sample per byte
                    load_window<34>(src.base, yo, my, ya);
                    if constexpr (CSTEP == 2) {
                        uint32_t ca[(CB + 3) / 4];
                        load_window<CB>(src.base, uo, mu, ca);
                        // pairs -> U0 U1 V0 V1 per dword, then the U halves and the V halves of two dwords together
                        const uint32_t sel = yp_swap ? 0x02000301u : 0x03010200u;
#pragma unroll
                        for (int i = 0; i < (CB + 3) / 4; ++i) ca[i] = __builtin_amdgcn_perm(0u, ca[i], sel);
#pragma unroll
                        for (int i = 0; i < (NC + 3) / 4; ++i) {
                            const uint32_t lo = ca[2 * i], hi = 2 * i + 1 < (CB + 3) / 4 ? ca[2 * i + 1] : 0u;
                            ua[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                            va[i] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
                        }
                    } else {
                        load_window<CB>(src.base, uo, mu, ua);
                        load_window<CB>(src.base, vo, mv, va);
                    }
                    uint32_t wl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // L' of the window's 34 pixels
#pragma unroll
                    for (int j = 0; j < NC; ++j) {
                        const int U = (int)((ua[j >> 2] >> ((j & 3) * 8)) & 255u), V = (int)((va[j >> 2] >> ((j & 3) * 8)) & 255u);
                        const YuvChroma c = yuv_chroma(U, V, mx);
                        const int cmax = yuv_cmax(c), cmin = yuv_cmin(c);
#pragma unroll
                        for (int q2 = 0; q2 < (SUBX ? 2 : 1); ++q2) {
                            const int k = SUBX ? 2 * j + q2 : j;
                            const int L = yuv_lightness((int)((ya[k >> 2] >> ((k & 3) * 8)) & 255u), cmax, cmin, mx);
                            wl[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                        }
                    }
                    // the lane's 32 pixels start at byte xodd of the window
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(wl[i + 1], wl[i], (uint32_t)xodd * 8u);
                } else {  // first / last bytes of the frame buffer: byte loads, the crop's own samples only
                    const uint8_t* py = src.base + fo + yp_yrow + (size_t)(src.x0 + xbeg);
                    const uint8_t* pu = src.base + fo + (size_t)yuv.u_off + yp_crow;
                    const uint8_t* pv = src.base + fo + (size_t)yuv.v_off + yp_crow;
                    for (int k = 0; k < npx; ++k) {
                        const int ci = ((src.x0 + xbeg + k) >> SUBX) * CSTEP;
                        const YuvChroma c = yuv_chroma(pu[ci], pv[ci], mx);
                        const int L = yuv_lightness(py[k], yuv_cmax(c), yuv_cmin(c), mx);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#elif defined(MELF_Y16_BODY)
            if (PX == 25) {
                const int xs = (src.x0 + xbeg) & ~1;   // the window's first pixel (even)
                const size_t fo = (size_t)f * src.frame_stride;
                const size_t yo = y16::prep_y_off(prow16, fo, xs);
                const size_t uo = y16::prep_c_off(prow16, fo, CSTEP == 2 ? prow16.c0 : (size_t)yuv.u_off, xs, CSTEP);   // CSTEP 2: the interleaved window
                const size_t vo = y16::prep_c_off(prow16, fo, (size_t)yuv.v_off, xs, CSTEP);                            // (CSTEP 1 only)
                const uint32_t my = (prow16.bm + (uint32_t)yo) & 3u, mu = (prow16.bm + (uint32_t)uo) & 3u, mv = (prow16.bm + (uint32_t)vo) & 3u;
                // the windows may reach past the crop and the row (never used: masked) but must stay inside the caller's buffer, at its
                // first bytes as well as at its last
                if (rows_safe || (y16::prep_window_ok(yo, my, y16::PREP_Y_BYTES, src.readable) && y16::prep_window_ok(uo, mu, CB, src.readable) &&
                                  (CSTEP == 2 || y16::prep_window_ok(vo, mv, CB, src.readable)))) {
                    uint32_t ya[9], ua[5], va[5];   // Y, U, V of the window reduced to 8 bits, a sample per byte
                    load_window16<34>(src.base, yo, my, y16_shift, ya);
                    if constexpr (CSTEP == 2) {
                        uint32_t ca[9];             // first, second, first, second .. of the pairs, a sample per byte
                        load_window16<34>(src.base, uo, mu, y16_shift, ca);
                        // pairs -> U0 U1 V0 V1 per dword, then the U halves and the V halves of two dwords together
                        const uint32_t sel = yp_swap ? 0x02000301u : 0x03010200u;
#pragma unroll
                        for (int i = 0; i < 9; ++i) ca[i] = __builtin_amdgcn_perm(0u, ca[i], sel);
#pragma unroll
                        for (int i = 0; i < 5; ++i) {
                            const uint32_t lo = ca[2 * i], hi = 2 * i + 1 < 9 ? ca[2 * i + 1] : 0u;
                            ua[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                            va[i] = __builtin_amdgcn_perm(hi, lo, 0x07060302u);
                        }
                    } else {
                        load_window16<17>(src.base, uo, mu, y16_shift, ua);
                        load_window16<17>(src.base, vo, mv, y16_shift, va);
                    }
                    uint32_t wl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // L' of the window's 34 pixels
#pragma unroll
                    for (int j = 0; j < 17; ++j) {
                        const int U = (int)((ua[j >> 2] >> ((j & 3) * 8)) & 255u), V = (int)((va[j >> 2] >> ((j & 3) * 8)) & 255u);
                        const YuvChroma c = yuv_chroma(U, V, mx);
                        const int cmax = yuv_cmax(c), cmin = yuv_cmin(c);
#pragma unroll
                        for (int q2 = 0; q2 < 2; ++q2) {
                            const int k = 2 * j + q2;
                            const int L = yuv_lightness((int)((ya[k >> 2] >> ((k & 3) * 8)) & 255u), cmax, cmin, mx);
                            wl[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                        }
                    }
                    // the lane's 32 pixels start at byte xodd of the window
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(wl[i + 1], wl[i], (uint32_t)xodd * 8u);
                } else {  // first / last bytes of the frame buffer: 2-byte loads, the crop's own samples only
                    const uint8_t* pf = src.base + fo;
                    for (int k = 0; k < npx; ++k) {
                        const int fx = src.x0 + xbeg + k;
                        const size_t co = y16::px_c_off(src.y0 + y, yuv.sub_y, (size_t)yuv.c_pitch, fx, CSTEP);
                        const YuvChroma c = yuv_chroma((int)y16::reduce(*(const uint16_t*)(pf + (size_t)yuv.u_off + co), y16_shift),
                                                       (int)y16::reduce(*(const uint16_t*)(pf + (size_t)yuv.v_off + co), y16_shift), mx);
                        const int L = yuv_lightness((int)y16::reduce(*(const uint16_t*)(pf + y16::px_y_off(src.y0 + y, (size_t)src.row_stride, fx)), y16_shift),
                                                    yuv_cmax(c), yuv_cmin(c), mx);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#elif defined(MELF_V210_BODY)
            if (PX == 26) {
                const int xs = (src.x0 + xbeg) & ~1;   // the window's first pixel (even)
                const int cnt = p10::v210_prep_groups(xs, src.x0 + xbeg + npx);   // groups that hold the lane's own pixels
                const int s = p10::v210_slot(xs);      // pair slot of the window's first pair in its group
                const u32x4m* q = (const u32x4m*)(src.base + p10::v210_prep_off((size_t)f * src.frame_stride, src.y0 + y, (size_t)src.row_stride, xs));
                u32x4m d[p10::V210_PREP_GROUPS];
                d[0] = q[0];
#pragma unroll
                for (int i = 1; i < p10::V210_PREP_GROUPS; ++i) {
                    d[i] = u32x4m{0u, 0u, 0u, 0u};
                    if ((i < 6 && rows_safe) || i < cnt) d[i] = q[i];
                }
                uint32_t pr[3 * p10::V210_PREP_GROUPS];   // every pair of the groups as Y0 U Y1 V
#pragma unroll
                for (int i = 0; i < 3 * p10::V210_PREP_GROUPS; ++i) {
                    const int g = i / 3, pq = i % 3;
                    const int iu = p10::pair_u(pq), iv = p10::pair_v(pq), iy0 = p10::pair_y(pq, 0), iy1 = p10::pair_y(pq, 1);
                    pr[i] = p10::field8(d[g][p10::field_word(iy0)], p10::field_bit(iy0)) | p10::field8(d[g][p10::field_word(iu)], p10::field_bit(iu)) << 8 |
                            p10::field8(d[g][p10::field_word(iy1)], p10::field_bit(iy1)) << 16 | p10::field8(d[g][p10::field_word(iv)], p10::field_bit(iv)) << 24;
                }
                uint32_t wl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // L' of the window's 34 pixels
#pragma unroll
                for (int j = 0; j < 17; ++j) {
                    const uint32_t m = s == 0 ? pr[j] : (s == 1 ? pr[j + 1] : pr[j + 2]);   // Y0 U Y1 V
                    const YuvChroma c = yuv_chroma((int)((m >> 8) & 255u), (int)(m >> 24), mx);
                    const int cmax = yuv_cmax(c), cmin = yuv_cmin(c);
                    const int L0 = yuv_lightness((int)(m & 255u), cmax, cmin, mx), L1 = yuv_lightness((int)((m >> 16) & 255u), cmax, cmin, mx);
                    wl[j >> 1] |= ((uint32_t)((L0 - 128) & 255) | (uint32_t)((L1 - 128) & 255) << 8) << ((j & 1) * 16);
                }
                // the lane's 32 pixels start at byte xodd of the window
#pragma unroll
                for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(wl[i + 1], wl[i], (uint32_t)xodd * 8u);
            } else
#elif defined(MELF_Y210_BODY)
            if (PX == 27) {
                const int xs = (src.x0 + xbeg) & ~1;   // the window's first pixel (even)
                const size_t o = p10::y210_prep_off((size_t)f * src.frame_stride, src.y0 + y, (size_t)src.row_stride, xs);
                // the window may reach past the crop and the row (never used: masked) but must stay inside the caller's buffer
                if (rows_safe || p10::y210_lane_ok(o, src.readable)) {
                    const u32x4a4* q = (const u32x4a4*)(src.base + o);
                    u32x4a4 d[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) d[i] = q[i];
                    const uint32_t d32 = ((const uint32_t*)(src.base + o))[32], d33 = ((const uint32_t*)(src.base + o))[33];
                    uint32_t wl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // L' of the window's 34 pixels
#pragma unroll
                    for (int j = 0; j < 17; ++j) {
                        const uint32_t lo = j < 16 ? d[j >> 1][(j & 1) * 2] : d32, hi = j < 16 ? d[j >> 1][(j & 1) * 2 + 1] : d33;   // Y0 U, Y1 V
                        const uint32_t m = __builtin_amdgcn_perm(hi, lo, 0x07050301u);   // the high bytes: Y0 U Y1 V
                        const YuvChroma c = yuv_chroma((int)((m >> 8) & 255u), (int)(m >> 24), mx);
                        const int cmax = yuv_cmax(c), cmin = yuv_cmin(c);
                        const int L0 = yuv_lightness((int)(m & 255u), cmax, cmin, mx), L1 = yuv_lightness((int)((m >> 16) & 255u), cmax, cmin, mx);
                        wl[j >> 1] |= ((uint32_t)((L0 - 128) & 255) | (uint32_t)((L1 - 128) & 255) << 8) << ((j & 1) * 16);
                    }
                    // the lane's 32 pixels start at byte xodd of the window
#pragma unroll
                    for (int i = 0; i < 8; ++i) w[i] = __builtin_amdgcn_alignbit(wl[i + 1], wl[i], (uint32_t)xodd * 8u);
                } else {  // last bytes of the frame buffer: one macropixel per pixel, inside the row
                    const uint8_t* pf = src.base + (size_t)f * src.frame_stride;
                    for (int k = 0; k < npx; ++k) {
                        const int fx = src.x0 + xbeg + k;
                        const uint32_t* mp = (const uint32_t*)(pf + p10::y210_px_off(src.y0 + y, (size_t)src.row_stride, fx));
                        const uint32_t sv = p10::y210_px_yuv(mp[0], mp[1], fx & 1);
                        const YuvChroma c = yuv_chroma((int)((sv >> 8) & 255u), (int)(sv >> 16), mx);
                        const int L = yuv_lightness((int)(sv & 255u), yuv_cmax(c), yuv_cmin(c), mx);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#elif defined(MELF_P32_BODY)
            if (PX == 28 || PX == 29) {
                const size_t o = prep::packed_x_off(src.x0 + xbeg, prep::packed_pb(4));
                const uint8_t* p = prow + o;
                // (as PX 4: the last block's window may reach past the crop, never past the caller's buffer)
                if (rows_safe || prep::packed_lane_ok(f, src.frame_stride, src.y0 + y, src.row_stride, o, prep::packed_win(4), src.readable)) {
                    const u32x4a4* q = (const u32x4a4*)p;
                    u32x4a4 d[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) d[i] = q[i];
#pragma unroll
                    for (int k = 0; k < 32; ++k) {
                        const uint32_t wd = d[k >> 2][k & 3];
                        int L;
                        if (PX == 28) {
                            const YuvChroma c = yuv_chroma((int)p32::read8(wd, fields.pos[1]), (int)p32::read8(wd, fields.pos[2]), mx);
                            L = yuv_lightness((int)p32::read8(wd, fields.pos[0]), yuv_cmax(c), yuv_cmin(c), mx);
                        } else {
                            L = hls_lightness_fast((int)p32::read8(wd, fields.pos[2]), (int)p32::read8(wd, fields.pos[1]), (int)p32::read8(wd, fields.pos[0]));
                        }
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                } else {  // last bytes of the frame buffer: one dword per pixel
                    for (int k = 0; k < npx; ++k) {
                        const uint32_t wd = ((const uint32_t*)p)[k];
                        int L;
                        if (PX == 28) {
                            const YuvChroma c = yuv_chroma((int)p32::read8(wd, fields.pos[1]), (int)p32::read8(wd, fields.pos[2]), mx);
                            L = yuv_lightness((int)p32::read8(wd, fields.pos[0]), yuv_cmax(c), yuv_cmin(c), mx);
                        } else {
                            L = hls_lightness((int)p32::read8(wd, fields.pos[2]), (int)p32::read8(wd, fields.pos[1]), (int)p32::read8(wd, fields.pos[0]));
                        }
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#elif defined(MELF_PLANAR_BODY)
            if (PX == 23) {
                // the lane's first sample in each plane, from the caller's base, and its byte phase there
                const size_t o = prep::planar_lane_off(f, src.frame_stride, src.y0 + y, src.row_stride, src.x0 + xbeg);
                const size_t ob = o + (size_t)planes.b_off, og = o + (size_t)planes.g_off, orr = o + (size_t)planes.r_off;
                const uint32_t mb = (pl_bm + (uint32_t)ob) & 3u, mg = (pl_bm + (uint32_t)og) & 3u, mr = (pl_bm + (uint32_t)orr) & 3u;
                // nine aligned dwords per plane cover its 32 bytes at any phase; the windows may reach past the crop and the row (never
                // used: masked) but must stay inside the caller's buffer, at its first bytes as well as at its last
                if (rows_safe || prep::planar_lane_ok(ob, mb, og, mg, orr, mr, src.readable)) {
                    const uint32_t* qb = (const uint32_t*)(src.base + (ob - mb));
                    const uint32_t* qg = (const uint32_t*)(src.base + (og - mg));
                    const uint32_t* qr = (const uint32_t*)(src.base + (orr - mr));
                    uint32_t db[9], dg[9], dr[9];
#pragma unroll
                    for (int i = 0; i < 9; ++i) { db[i] = qb[i]; dg[i] = qg[i]; dr[i] = qr[i]; }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        // four pixels: their B, G and R samples, one dword each
                        const uint32_t B = __builtin_amdgcn_alignbit(db[i + 1], db[i], mb * 8u), G = __builtin_amdgcn_alignbit(dg[i + 1], dg[i], mg * 8u),
                                       Rr = __builtin_amdgcn_alignbit(dr[i + 1], dr[i], mr * 8u);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int L = hls_lightness_fast((B >> (8 * k)) & 255, (G >> (8 * k)) & 255, (Rr >> (8 * k)) & 255);
                            w[i] |= (uint32_t)((L - 128) & 255) << (8 * k);
                        }
                    }
                } else {  // first / last bytes of the frame buffer: byte loads, the crop's own samples only
                    const uint8_t* pb = src.base + ob;
                    const uint8_t* pg = src.base + og;
                    const uint8_t* pr = src.base + orr;
                    for (int k = 0; k < npx; ++k) {
                        const int L = hls_lightness(pb[k], pg[k], pr[k]);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else
#endif
            if (PX == 3) {
                const size_t o = prep::packed_x_off(src.x0 + xbeg, 3);
                const uint8_t* p = prow + o;
                const int mis = (int)((size_t)p & 3);
                // 25 aligned dwords cover the 96 bytes of 32 pixels at any byte alignment; the window may
                // reach past the crop (never used: masked) but must stay inside the caller's buffer
                if (rows_safe || prep::packed_lane_ok(f, src.frame_stride, src.y0 + y, src.row_stride, o, 100, src.readable)) {
                    const uint32_t* q = (const uint32_t*)(p - mis);
                    uint32_t d[25];
#pragma unroll
                    for (int i = 0; i < 25; ++i) d[i] = q[i];
                    uint32_t a[24];
#pragma unroll
                    for (int i = 0; i < 24; ++i) a[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], (uint32_t)mis * 8u);
#pragma unroll
                    for (int k = 0; k < 32; ++k) {
                        const int j = (3 * k) >> 2, sh = ((3 * k) & 3) * 8;
                        const uint32_t px = sh <= 8 ? (a[j] >> sh) : __builtin_amdgcn_alignbit(a[j + 1 < 24 ? j + 1 : 23], a[j], sh);
                        const int L = hls_lightness_fast(px & 255, (px >> 8) & 255, (px >> 16) & 255);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                    // (The last block's columns beyond the image keep whatever the gather found there -- pixels of the same frame.  No map
                    // position inside the map reaches them: x + j <= cols - 1 for x < rw, and the window sums stop at column cols - 1 too;
                    // the positions that do are thrown away by the match kernels.  Masking them cost 40 issue slots per wave and row.)
                } else {  // last bytes of the frame buffer: byte loads
                    for (int k = 0; k < npx; ++k) {
                        const int L = hls_lightness(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else if (PX == 4) {
                const size_t o = prep::packed_x_off(src.x0 + xbeg, 4);
                const uint8_t* p = prow + o;
                // (as above: the last block's window may reach past the crop, never past the caller's buffer)
                if (rows_safe || prep::packed_lane_ok(f, src.frame_stride, src.y0 + y, src.row_stride, o, 128, src.readable)) {
                    const u32x4a4* q = (const u32x4a4*)p;
                    u32x4a4 d[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) d[i] = q[i];
#pragma unroll
                    for (int k = 0; k < 32; ++k) {
                        const uint32_t px = d[k >> 2][k & 3];
                        const int L = hls_lightness_fast(px & 255, (px >> 8) & 255, (px >> 16) & 255);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                } else {  // last bytes of the frame buffer: one dword per pixel
                    for (int k = 0; k < npx; ++k) {
                        const uint32_t px = ((const uint32_t*)p)[k];
                        const int L = hls_lightness(px & 255, (px >> 8) & 255, (px >> 16) & 255);
                        w[k >> 2] |= (uint32_t)((L - 128) & 255) << ((k & 3) * 8);
                    }
                }
            } else {
                const uint8_t* p = prow + src.x0 + xbeg;
                for (int k = 0; k < npx; ++k) w[k >> 2] |= (uint32_t)(((int)p[k] - 128) & 255) << ((k & 3) * 8);
            }
        }
        if (kc) __syncthreads();  // the previous chunk's tile has been written out
        // fragment-order image of the row (plain: the paired operands are put together when the row leaves, below)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            u32x4m v = {w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
            *(u32x4m*)(tile + ((kl * 2 + h) * 32 + n) * 4) = v;
        }
        // inclusive prefix sums of L' along the row: the block's total (four signed bytes per v_dot4), a scan of the totals over the
        // frame's 8 lanes, then the 32 running sums are produced and stored pair by pair (nothing but the running sum stays live)
        int run = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) run = __builtin_amdgcn_sdot4((int)w[j], 0x01010101, run, false);
        int off = run;  // inclusive scan of block totals over lanes with equal t >> 3
#pragma unroll
        for (int dlt = 1; dlt < 8; dlt <<= 1) {
            const int o2 = __shfl_up(off, dlt, 8);
            if (kl >= dlt) off += o2;
        }
        const int chunk_total = __shfl(off, 7, 8);
        off += carry - run;  // exclusive, including the earlier chunks
        carry += chunk_total;
        if (kb < nkb) {
            int acc = off;
#pragma unroll
            for (int k = 0; k < 32; k += 2) {
                acc += (int)(int8_t)((w[k >> 2] >> ((k & 3) * 8)) & 255u);
                const uint32_t lo16 = (uint32_t)acc & 0xffffu;
                acc += (int)(int8_t)((w[k >> 2] >> (((k + 1) & 3) * 8)) & 255u);
                *(uint32_t*)&pre_dyn[n * pstride + kb * 32 + k] = lo16 | ((uint32_t)acc << 16);
            }
        }
        __syncthreads();
        const int nb = min(8, nkb - kc);
        if (pairs == 0) {
            for (int i = t; i < nb * 64; i += 256) out[kc * 64 + i] = *(const u32x4m*)(tile + i * 4);
        } else {
            // (nkb <= 8: one chunk)  output piece i = 1 KiB slot i >> 6, lane i & 63.  Slots 2 p, 2 p + 1: dwords 0-3 / 4-7 of P_p -- two
            // dwords of block p's fragment and two of block p + 6's, interleaved by 16-bit pairs; slots 2 pairs ..: blocks pairs .. 5
            for (int i = t; i < nb * 64; i += 256) {
                const int slot = i >> 6, li = i & 63;
                u32x4m v;
                if (slot < 2 * pairs) {   // (uniform per wave)
                    const int p = slot >> 1, hl = slot & 1;
                    const uint2 lo2 = *(const uint2*)(tile + (p * 64 + li) * 4 + 2 * hl), hi2 = *(const uint2*)(tile + ((p + 6) * 64 + li) * 4 + 2 * hl);
                    v.x = __builtin_amdgcn_perm(hi2.x, lo2.x, 0x05040100u); v.y = __builtin_amdgcn_perm(hi2.x, lo2.x, 0x07060302u);
                    v.z = __builtin_amdgcn_perm(hi2.y, lo2.y, 0x05040100u); v.w = __builtin_amdgcn_perm(hi2.y, lo2.y, 0x07060302u);
                } else {
                    v = *(const u32x4m*)(tile + ((slot - pairs) * 64 + li) * 4);
                }
                out[i] = v;
            }
        }
    }
    // window sums: R[x] = P[x + tw - 1] - P[x - 1] + 128 tw   (P = inclusive prefix of L - 128, modulo 2^16:
    // the window sum itself is below 2^16 for tw <= 257)
    if (y < src.rows) {
        uint16_t* ro = R + (((size_t)grp * src.rows + y) * rwp) * 32;
        const int bias = tw * 128;
        const int pmax = nkb * 32 - 1;
        const int ln = t & 63, nn = ln & 31, hh = ln >> 5;
        for (int kk = t >> 6; kk < rwp / 16; kk += 4) {   // 1 KiB pieces, four per pass of the workgroup
            const int xb = kk >> 1, e0 = 8 * (kk & 1);
            uint32_t o[4];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int e = e0 + q;
                const int x = 32 * xb + (e & 3) + 8 * (e >> 2) + 4 * hh;
                const int hi = (int)pre_dyn[nn * pstride + min(x + tw - 1, pmax)], lo = x > 0 ? (int)pre_dyn[nn * pstride + min(x - 1, pmax)] : 0;
                const uint32_t v = (uint32_t)(hi - lo + bias) & 0xffffu;
                if (q & 1) o[q >> 1] |= v << 16; else o[q >> 1] = v;
            }
            u32x4m ov = {o[0], o[1], o[2], o[3]};
            *(u32x4m*)(ro + ((size_t)kk * 64 + ln) * 8) = ov;
        }
    }
