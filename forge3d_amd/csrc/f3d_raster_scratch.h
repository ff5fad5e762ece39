// f3d_raster_scratch.h -- where the pieces of a host-form raster call lie in the session's scratch: plain arithmetic, no HIP
// type (tests/raster_scratch_host compiles it alone).  A call is an ordered list of segments -- its outputs and its one input;
// they are laid out in the order given, back to back, and the input starts on a multiple of 16 (its rows are read as float4
// or float2).  An absent segment has 0 bytes: it takes no room, but an input still rounds.  The five lists (f3d_host_rasters.h):
//   raster       masks, [targets], count            horizon    planes, sky_view, [azimuths]
//   irradiation  energy, count, normals, [directions]   clearance  planes, lowest, [observers]
//   umbra        planes, deepest, [directions]
#pragma once

#include <cstddef>
#include <cstdint>

struct ScratchSegment {
    uint64_t bytes;
    bool input;
    uint64_t offset;  // filled in by scratch_layout
};

// Fills in every segment's offset and returns the bytes the call needs.
inline uint64_t scratch_layout(ScratchSegment *segments, size_t count) {
    uint64_t at = 0u;
    for (size_t i = 0; i < count; i++) {
        if (segments[i].input) at = (at + 15u) & ~(uint64_t)15u;
        segments[i].offset = at;
        at += segments[i].bytes;
    }
    return at;
}
