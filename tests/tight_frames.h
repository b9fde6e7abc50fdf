// For the bounds programs (y16_bounds_main.cpp, prep_bounds_main.cpp, frame_src_bounds_main.cpp): a public descriptor through its
// check (meterelf_amd/csrc/melf_frame_checks.h) as an entry point calls it, at the smallest frame_stride the check takes plus spad
// bytes.  Leaves the batch the launchers would be handed in *b and returns the check's message if the descriptor is not taken.
#pragma once
#include <stdint.h>

#include "../meterelf_amd/csrc/melf_frame_checks.h"

template <class D, class Check>
static const char* tight_frames(const Check& check, D& d, int64_t spad, size_t phase, melf::FrameBatch* b)
{
    const void* const base = (const void*)(uintptr_t)(4096 + phase);   // never read: the check looks at NULL and alignment only
    d.frame_stride = INT64_MAX & ~(int64_t)3;                          // any stride: the check leaves the extent of one frame
    const char* msg = check(base, &d, b);
    if (msg) return msg;
    d.frame_stride = (int64_t)b->lay.extent + spad;
    return check(base, &d, b);
}
