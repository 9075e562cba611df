"""GPU: the batched strided block copy (csrc/copy_blocks.hip, ops.copy_blocks) against torch indexing, bit for bit over whole
buffers: block sizes around the tile, dense and wide strides, tables of 1, 2 and 64 entries with empty ones among them, the K/V
cache shape packed and unpacked, offsets beyond 4 GiB and a non-default stream.  Destinations are pre-filled with a pattern, so a
stray write shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu
U8, F16 = torch.uint8, torch.float16


def _tile():
    from fs_eend_amd import ops
    return ops.copy_blocks_tile_bytes()


def _bytes(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n,), generator=g, dtype=U8).to(dev)


def _pattern(n, dev):
    return ((torch.arange(n, device=dev) * 7 + 3) % 251).to(U8)


def _expect(dst, src, nblocks, block_bytes, ss, ds, s0=0, d0=0):
    """dst (uint8, in place) after the entry, by torch indexing"""
    for b in range(nblocks):
        dst[d0 + b * ds:d0 + b * ds + block_bytes] = src[s0 + b * ss:s0 + b * ss + block_bytes]


def _sizes():
    tile = _tile()
    return [16, 128, tile - 16, tile, tile + 16, 3 * tile + 48]


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "wide"])
@pytest.mark.parametrize("nblocks", [1, 2, 5])
@pytest.mark.parametrize("size", range(6), ids=["16", "128", "tile-16", "tile", "tile+16", "3tile+48"])
def test_block_sizes_and_strides(hip_lib, dev, size, nblocks, wide):
    from fs_eend_amd import ops
    bb = _sizes()[size]
    ss, ds = (bb + 48, bb + 272) if wide else (bb, bb)
    src = _bytes(64 + nblocks * ss, 100 + size, dev)
    dst = _pattern(128 + nblocks * ds, dev)
    keep, want = src.clone(), dst.clone()
    _expect(want, src, nblocks, bb, ss, ds, 32, 48)
    ops.copy_blocks([(src.data_ptr() + 32, dst.data_ptr() + 48, nblocks, bb, ss, ds)])
    torch.cuda.synchronize()
    assert torch.equal(dst, want) and torch.equal(src, keep)


@pytest.mark.parametrize("n", [1, 2, 64])
def test_tables_of_mixed_entries(hip_lib, dev, n):
    """n entries of mixed sizes into one destination buffer, every third one empty (no blocks, or blocks of no bytes)."""
    from fs_eend_amd import ops
    tile = _tile()
    sizes = [16, 48, 128, 1024, tile - 16, tile, tile + 16, 2 * tile + 32]
    entries, plan, s_off, d_off = [], [], 16, 64
    for i in range(n):
        bb, nb = sizes[i % len(sizes)], 1 + i % 4
        if i % 3 == 2:
            bb, nb = (0, nb) if i % 2 else (bb, 0)
        ss, ds = bb + 16 * (i % 3), bb + 32 * (i % 2)
        plan.append((nb, bb, ss, ds, s_off, d_off))
        s_off += nb * ss + 16
        d_off += nb * ds + 48
    src, dst = _bytes(s_off, n, dev), _pattern(d_off, dev)
    keep, want = src.clone(), dst.clone()
    for nb, bb, ss, ds, so, do in plan:
        empty = nb == 0 or bb == 0
        entries.append((0 if empty and nb == 0 else src.data_ptr() + so, dst.data_ptr() + do, nb, bb, ss, ds))
        _expect(want, src, nb, bb, ss, ds, so, do)
    ops.copy_blocks(entries)
    torch.cuda.synchronize()
    assert torch.equal(dst, want) and torch.equal(src, keep)
    assert n == 1 or not torch.equal(dst, _pattern(d_off, dev))


@pytest.fixture(scope="module")
def kcache(dev):
    g = torch.Generator().manual_seed(9)
    return torch.randn(18, 4, 128, 64, generator=g).to(F16).to(dev)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 127, 128])
def test_cache_rows_pack_and_unpack(hip_lib, dev, kcache, n):
    """Rows [0, n) of sequences 6..11 of a (18, 4, 128, 64) f16 K cache -> a packed blob -> sequences 12..17 of a (24, 4, 256, 64)
    cache: the blob is k[6:12, :, :n].contiguous(), and exactly those rows of the second cache change."""
    from fs_eend_amd import ops
    k = kcache
    keep = k.clone()
    H, row = 4, 128
    blob = torch.full((6, H, n, 64), 7.0, dtype=F16, device=dev)
    guard = torch.full((4096,), 5, dtype=U8, device=dev)           # allocated next: a write past the blob lands nearby
    ops.copy_blocks([(k[6].data_ptr(), blob.data_ptr(), 6 * H, n * row, 128 * row, n * row)])
    torch.cuda.synchronize()
    assert torch.equal(blob, k[6:12, :, :n].contiguous()) and torch.equal(k, keep)
    assert bool((guard == 5).all())
    big = torch.full((24, H, 256, 64), -3.0, dtype=F16, device=dev)
    want = big.clone()
    want[12:18, :, :n] = k[6:12, :, :n]
    ops.copy_blocks([(blob.data_ptr(), big[12].data_ptr(), 6 * H, n * row, n * row, 256 * row)])
    torch.cuda.synchronize()
    assert torch.equal(big, want)


def test_offsets_beyond_4_gib(hip_lib, dev):
    """Two 4 KiB blocks at a stride of 2^32 + 4096 bytes, out of and into a buffer of more than 4 GiB that is only allocated: a
    32-bit offset would wrap the second block onto byte 4096."""
    from fs_eend_amd import ops
    stride, bb = (1 << 32) + 4096, 4096
    big = torch.empty(stride + 2 * bb, dtype=U8, device=dev)
    a, b = _bytes(bb, 1, dev), _bytes(bb, 2, dev)
    big[:bb], big[bb:2 * bb], big[stride:stride + bb] = a, _pattern(bb, dev), b
    out = _pattern(3 * bb, dev)
    want = out.clone()
    want[:bb], want[bb:2 * bb] = a, b
    ops.copy_blocks([(big.data_ptr(), out.data_ptr(), 2, bb, stride, bb)])     # gather: source offsets beyond 2^32
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    c, d = _bytes(bb, 3, dev), _bytes(bb, 4, dev)
    pair = torch.cat([c, d])
    big[stride + bb:stride + 2 * bb] = _pattern(bb, dev)
    ops.copy_blocks([(pair.data_ptr(), big.data_ptr(), 2, bb, bb, stride)])    # scatter: destination offsets beyond 2^32
    torch.cuda.synchronize()
    assert torch.equal(big[:bb], c) and torch.equal(big[bb:2 * bb], _pattern(bb, dev))
    assert torch.equal(big[stride:stride + bb], d) and torch.equal(big[stride + bb:], _pattern(bb, dev))


def test_on_a_non_default_stream(hip_lib, dev):
    from fs_eend_amd import ops
    tile = _tile()
    bb = 2 * tile + 16
    src, dst = _bytes(3 * bb, 11, dev), _pattern(3 * (bb + 64), dev)
    want = dst.clone()
    _expect(want, src, 3, bb, bb, bb + 64)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        ops.copy_blocks([(src.data_ptr(), dst.data_ptr(), 3, bb, bb, bb + 64)])
    st.synchronize()
    assert torch.equal(dst, want)


def test_nothing_to_move_and_bad_entries(hip_lib, dev):
    from fs_eend_amd import ops
    from fs_eend_amd.lib import EendHipError
    dst = _pattern(256, dev)
    ops.copy_blocks([])
    ops.copy_blocks([(0, dst.data_ptr(), 0, 64, 0, 0), (dst.data_ptr(), dst.data_ptr(), 4, 0, 0, 0)])
    with pytest.raises(EendHipError, match="eend_copy_blocks"):
        ops.copy_blocks([(dst.data_ptr(), dst.data_ptr() + 32, 1, 64, 0, 0)])              # overlapping ranges
    with pytest.raises(EendHipError, match="eend_copy_blocks"):
        ops.copy_blocks([(dst.data_ptr(), dst.data_ptr() + 128, 1, 24, 0, 0)])             # not a multiple of 16
    torch.cuda.synchronize()
    assert torch.equal(dst, _pattern(256, dev))
