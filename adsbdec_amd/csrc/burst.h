// burst.h -- the launches of burst_kernel.hip: the gate behind the envelope (include/adsbdec_amd.h: adsb_bursts_*;
// decoder_bursts.hip).  An envelope of R floats -> the ordered table of its bursts; adsbdec_amd/levels.py bursts is the definition.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#pragma GCC visibility push(hidden)

namespace adsb {

constexpr uint32_t kBurstTileRuns = 2048;   // T: consecutive runs of one tile, one workgroup of 256 lanes, 8 runs a lane
constexpr uint32_t kBurstNone = 0xFFFFFFFFu; // "no hot run" (a run index stays below 2^31 + 3)
constexpr int kBurstTileWords = 4;           // a tile's summary {first, last, inner starts, 0} and its combine row {before, after, first is a start, starts before}

// What the three launches share.  The envelope is read through its 16-byte grid: `base` is env rounded DOWN to 16 bytes and `pad`
// (0 .. 3) the floats between the two, so grid index v = r + pad holds run r and a lane's quads are aligned whatever env is; the
// quad that holds env[0] and the one that holds env[R - 1] are read float by float where they reach outside the envelope.  Tiles
// are cut on the grid: with a 16-byte aligned envelope tile t is the runs [t T, (t + 1) T), else its seams lie `pad` runs earlier.
struct BurstArgs {
    const float *base;
    uint32_t pad, runs;        // R = runs
    uint32_t threshold_bits;   // hot: u >= threshold_bits
    uint32_t lead, hang, join; // join = lead + hang + 1
    uint32_t n_tiles;          // ceil((R + pad) / T)
    uint32_t *summaries;       // n_tiles x kBurstTileWords
    uint32_t *rows;            // n_tiles x kBurstTileWords
    uint32_t *total;           // B
    uint32_t *table;           // cap records of 4 words {begin, end, hot, peak bits}, zeroed on the same stream before the emit
    uint32_t cap;
};

// What the launches of a SLICE of a stream take besides (burst_slice_kernel.hip; adsb_bursts_slice_*): run r of the slice is run
// first_run + r of the stream, and every run the kernels hold or write is a stream run.  The cluster that earlier slices left
// open is burst 0 of the slice: its last hot run + 1 (0: none is open) is the hot run before tile 0, and it is the one start in
// front of the slice.  The table has cap + 1 records: the bursts k < cap as {max(0, first - lead), last + hang + 1, hot, peak},
// and behind them the LAST burst, k = B - 1, as {first, last + 1, hot, peak}; cap <= B - 1.  Of the carried cluster the kernels
// write only what the slice adds: its begin stays 0, its end too where no hot run of the slice joins it, and the host sees to both.
struct BurstSlice {
    uint32_t first_run, prev_last1, prev_starts;
};

inline uint32_t burst_tiles(uint64_t runs, uint32_t pad) { return (uint32_t)((runs + pad + kBurstTileRuns - 1) / kBurstTileRuns); }

// The summaries of every tile, then the combine (one workgroup): rows and *total are complete when the stream reaches what follows.
hipError_t launch_burst_count(const BurstArgs &a, hipStream_t stream);
// The emit: the records k < cap of the table.  The table holds zeroes when it starts.
hipError_t launch_burst_emit(const BurstArgs &a, hipStream_t stream);
// The same two of a slice (burst_slice_kernel.hip): *total counts the carried cluster; the table's cap + 1 records hold zeroes.
hipError_t launch_burst_slice_count(const BurstArgs &a, const BurstSlice &s, hipStream_t stream);
hipError_t launch_burst_slice_emit(const BurstArgs &a, const BurstSlice &s, hipStream_t stream);

} // namespace adsb

#pragma GCC visibility pop
