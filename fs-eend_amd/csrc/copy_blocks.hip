// Batched strided block copy: every piece of a stream slot's state -- the K/V rows of each layer up to the slot's history length,
// the retention states, the conv caches, the look-ahead window -- moved between the session's buffers and one contiguous snapshot
// blob by ONE launch, in either direction (MultiStreamSession.snapshot / resume).
//
// A piece is "nblocks blocks of block_bytes, at a source stride and a destination stride".  The entries travel by value in the
// kernel arguments (at most CB_MAX of them: 64 x 48 B + the tile tables = 3.6 KB, under the 4 KB argument block), so there is no
// device table, no staging copy and nothing to keep alive; every check happens on the host before the launch.
//
// Work is cut into tiles of CB_TILE bytes that never span two blocks: a block of b bytes has ceil(b / CB_TILE) tiles, the last
// one short.  Tiles are numbered entry by entry; tile_end[e] is the running total, so a workgroup finds the entry of tile g with
// a scan of at most n uniform compares, then block = local / tiles_per_block.  A workgroup of 256 lanes moves a tile as CB_UNROLL
// rounds of one 16-byte load and store per lane (all loads of a tile in flight before its first store), and the grid -- a few
// workgroups per compute unit -- strides over the tiles.  Byte offsets are 64-bit throughout: one blob may exceed 4 GiB.
#include "kernels.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int CB_THREADS = 256, CB_UNROLL = 4;
constexpr long CB_TILE = (long)CB_THREADS * 16 * CB_UNROLL;          // 16 KiB per workgroup and tile

struct CopyArgs {
    eend_block_copy e[EEND_COPY_BLOCKS_MAX];
    unsigned tile_end[EEND_COPY_BLOCKS_MAX];                          // tiles of entries 0..e, inclusive (empty entries add none)
    unsigned tiles_per_block[EEND_COPY_BLOCKS_MAX];
    int n;
};
static_assert(sizeof(CopyArgs) + 8 <= 4096, "the entries travel in the kernel arguments");

__global__ __launch_bounds__(CB_THREADS) void copy_blocks_kernel(const CopyArgs a, const unsigned total) {
    for (unsigned g = blockIdx.x; g < total; g += gridDim.x) {
        int e = 0;
        while (g >= a.tile_end[e]) ++e;                               // uniform; g < total = tile_end[n - 1] ends it inside the table
        const unsigned local = g - (e ? a.tile_end[e - 1] : 0u);
        const unsigned tpb = a.tiles_per_block[e];
        const unsigned blk = local / tpb, tile = local - blk * tpb;
        const long off = (long)tile * CB_TILE;                        // inside the block
        const long left = a.e[e].block_bytes - off;                   // > 0; a multiple of 16
        const char* src = (const char*)a.e[e].src + (long)blk * a.e[e].src_stride + off;
        char* dst = (char*)a.e[e].dst + (long)blk * a.e[e].dst_stride + off;
        u32x4 v[CB_UNROLL];
#pragma unroll
        for (int j = 0; j < CB_UNROLL; ++j) {
            const long o = ((long)j * CB_THREADS + threadIdx.x) * 16;
            if (o < left) v[j] = *(const u32x4*)(src + o);
        }
#pragma unroll
        for (int j = 0; j < CB_UNROLL; ++j) {
            const long o = ((long)j * CB_THREADS + threadIdx.x) * 16;
            if (o < left) *(u32x4*)(dst + o) = v[j];
        }
    }
}

}  // namespace

long eend_copy_blocks_tile() { return CB_TILE; }

// entries: validated by the caller (api.hip): non-negative 16-byte multiples, non-null pointers where bytes move.
int eend_launch_copy_blocks(const eend_block_copy* entries, int n, hipStream_t stream) {
    CopyArgs a;
    unsigned long total = 0;
    a.n = n;
    for (int i = 0; i < EEND_COPY_BLOCKS_MAX; ++i) {
        unsigned long tpb = 0, tiles = 0;
        if (i < n) {
            a.e[i] = entries[i];
            if (entries[i].nblocks > 0 && entries[i].block_bytes > 0) {
                tpb = ((unsigned long)entries[i].block_bytes + CB_TILE - 1) / CB_TILE;
                if (tpb > 0x7fffffffUL || (unsigned long)entries[i].nblocks > 0x7fffffffUL / tpb) return EEND_EINVAL;
                tiles = tpb * (unsigned long)entries[i].nblocks;
            }
        } else {
            a.e[i] = eend_block_copy{nullptr, nullptr, 0, 0, 0, 0};
        }
        total += tiles;
        if (total > 0x7fffffffUL) return EEND_EINVAL;                 // 2^31 tiles = 32 TiB: no such copy
        a.tile_end[i] = (unsigned)total;
        a.tiles_per_block[i] = tpb ? (unsigned)tpb : 1u;
    }
    if (total == 0) return EEND_OK;                                   // nothing to move (a fresh slot): no launch
    const unsigned long cap = (unsigned long)eend_cu_count() * 8;
    const unsigned grid = (unsigned)(total < cap ? total : cap);
    hipLaunchKernelGGL(copy_blocks_kernel, dim3(grid), dim3(CB_THREADS), 0, stream, a, (unsigned)total);
    return hipGetLastError() == hipSuccess ? EEND_OK : EEND_ELAUNCH;
}
