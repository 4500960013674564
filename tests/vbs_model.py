"""The block-size search's rules restated in Python for the tests (include/flacenc_hip.h, flacenc_hip_encode_variable):
the coded number of RFC 9639 section 9.1.5, the tree minimum over a superblock's dyadic tilings, the bounds."""


def coded_number(v: int) -> bytes:
    """RFC 9639 section 9.1.5: the UTF-8-like code of v < 2^36."""
    assert 0 <= v < 1 << 36
    if v < 0x80:
        return bytes([v])
    for n, bits in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31), (7, 36)):
        if v < 1 << bits:
            break
    tail = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 1)][::-1]
    lead = (0xFF00 >> n) & 0xFF | (v >> (6 * (n - 1)))
    return bytes([lead] + tail)


def tree_min(lens, levels):
    """lens[n], heap nodes n = 1 .. 2^levels - 1 -> (best total, split mask of the chosen tiling, its nodes in order).
    Node n is split exactly when its children's best sum is strictly below lens[n]."""
    first_leaf = 1 << (levels - 1)
    best, split = {}, set()
    for n in range((1 << levels) - 1, 0, -1):
        best[n] = lens[n]
        if n < first_leaf and best[2 * n] + best[2 * n + 1] < lens[n]:
            best[n] = best[2 * n] + best[2 * n + 1]
            split.add(n)
    mask, leaves = 0, []

    def walk(n):
        nonlocal mask
        if n in split:
            mask |= 1 << (n - 1)
            walk(2 * n)
            walk(2 * n + 1)
        else:
            leaves.append(n)

    walk(1)
    return best[1], mask, leaves


def node_level(n):
    return n.bit_length() - 1


def frame_bound(channels, block, bps):
    """The fixed-blocking frame bound (csrc/frame_pack.cpp, before rounding to 16 bytes)."""
    if channels == 2:
        return 15 + (16 + block * (2 * bps + 1) + 7) // 8 + 2
    return 15 + (channels * (8 + block * bps) + 7) // 8 + 2


def variable_bytes_bound(channels, block_size, levels, bps, total):
    n_full, tail = divmod(total, block_size)
    return n_full * (frame_bound(channels, block_size, bps) + 1) + (frame_bound(channels, tail, bps) + 1 if tail else 0)


def variable_max_frames(block_size, levels, total):
    n_full, tail = divmod(total, block_size)
    return (n_full << (levels - 1)) + (1 if tail else 0)
