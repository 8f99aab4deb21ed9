// gci_site_tiles.hpp -- the tile of a window that the site listers walk (k_indels.hip, k_mismatch.hip): K8's windows cut into
// 4096-element tiles, one workgroup each; which of the tile's elements lie inside the window and inside their contig, and where a
// run that begins in the tile may begin and must end.
#pragma once
#include "gci_ctx.hpp"

struct SiteTile {
    int64_t p0;                          // the tile's first element (a multiple of TILE)
    int64_t lo, hi;                      // the elements of the tile that are inside the window AND inside their contig
    int64_t run_lo, run_hi;              // ... of the whole track: where a run of this tile may begin and must end
    int64_t contig_off;
    int32_t contig;
};

__device__ __forceinline__ SiteTile site_tile_of(const gci_window* __restrict__ win, const int64_t* __restrict__ win_tile_first, int32_t n_win,
                                                   int64_t wt, const int64_t* __restrict__ off, const int64_t* __restrict__ len,
                                                   const int64_t* __restrict__ tile_first, int32_t n_contigs)
{
    SiteTile x;
    const int32_t w = contig_of_tile(win_tile_first, n_win, wt);
    const gci_window W = win[w];
    x.p0 = (W.begin / TILE + (wt - win_tile_first[w])) * TILE;
    x.contig = contig_of_tile(tile_first, n_contigs, x.p0 / TILE);
    x.contig_off = off[x.contig];
    x.run_lo = max(W.begin, x.contig_off);
    x.run_hi = min(W.end, x.contig_off + len[x.contig]);
    x.lo = max(x.p0, x.run_lo);
    x.hi = min(x.p0 + TILE, x.run_hi);
    return x;
}
