// stage_layout.hpp -- where the captures of a batch lie in one buffer of the handle's (batch_in, batch_land, batch_unpacked): side by
// side in capture order, each at a multiple of `align` bytes.  Host-only and pure: decoder_stage.hip lays every batch buffer out with
// it, and tests/cpp/stage_layout.cpp holds it to a plain restatement.
#pragma once

#include <stddef.h>

namespace adsb {

// off[i] = the sum of bytes[0 .. i), each rounded up to `align` (a power of two).  Returns the total: where a further capture would
// start.  A capture without bytes takes no room: it starts where the next one does.
inline size_t stage_layout(size_t n_captures, const size_t *bytes, size_t align, size_t *off)
{
    size_t at = 0;
    for (size_t i = 0; i < n_captures; i++) {
        off[i] = at;
        at += (bytes[i] + align - 1) & ~(align - 1);
    }
    return at;
}

} // namespace adsb
