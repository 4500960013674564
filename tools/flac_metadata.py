"""The metadata blocks of a .flac file on the host, in plain Python (no GPU, no numpy): STREAMINFO and SEEKTABLE read
(tools/decode_flac.py, tools/decode_many.py and tools/crop_flac.py share this reader) and the SEEKTABLE block built
(tools/encode_flac.py --seektable).  RFC 9639 section 8.5: a seek point is 18 bytes -- the sample number of the first
sample of its target frame (64 bits), the byte offset of that frame from the first frame (64 bits) and its block size
(16 bits), big-endian, in ascending order; a placeholder point has the sample number 0xFFFFFFFFFFFFFFFF."""
import struct

PLACEHOLDER = 0xFFFFFFFFFFFFFFFF
SEEKTABLE = 3


def parse_seektable(body: bytes):
    """-> [(sample number, byte offset from the first frame, block size)], placeholder points included."""
    if len(body) % 18:
        raise ValueError("a SEEKTABLE block is a whole number of 18-byte points")
    return [struct.unpack(">QQH", body[at:at + 18]) for at in range(0, len(body), 18)]


def seektable_block(points, last=True) -> bytes:
    """The whole metadata block (header included) of the given (sample number, byte offset, block size) points."""
    body = b"".join(struct.pack(">QQH", int(s), int(o), int(b)) for s, o, b in points)
    return bytes([SEEKTABLE | (0x80 if last else 0)]) + len(body).to_bytes(3, "big") + body


def seek_points(frame_lengths, block_sizes, every_samples):
    """One point per `every_samples` samples from the frames' byte lengths and block sizes: the frame that holds sample
    k * every_samples, each frame at most once, the first frame always."""
    if every_samples < 1:
        raise ValueError("the spacing of seek points is at least one sample")
    points, sample, offset, want = [], 0, 0, 0
    for length, bs in zip(frame_lengths, block_sizes):
        length, bs = int(length), int(bs)
        if sample + bs > want:   # this frame holds sample `want`
            points.append((sample, offset, bs))
            want = (sample + bs + every_samples - 1) // every_samples * every_samples
        sample += bs
        offset += length
    return points


def last_point_at_or_before(points, sample):
    """The last non-placeholder point whose sample number is <= sample, or (0, 0, 0): the first frame."""
    best = (0, 0, 0)
    for p in points or ():
        if p[0] != PLACEHOLDER and best[0] <= p[0] <= sample:
            best = tuple(p)
    return best


def read_blocks(data: bytes):
    """-> (STREAMINFO fields, the SEEKTABLE's points or None, byte offset of the first frame)."""
    if data[:4] != b"fLaC":
        raise ValueError("not a FLAC stream")
    pos, info, points = 4, None, None
    while True:
        head = data[pos]
        kind, size = head & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + size]
        if kind == 0:
            max_block = struct.unpack(">H", body[2:4])[0]
            packed = int.from_bytes(body[10:18], "big")
            info = dict(max_block_size=max_block, sample_rate=packed >> 44, channels=((packed >> 41) & 7) + 1,
                        bits_per_sample=((packed >> 36) & 31) + 1, total_samples=packed & ((1 << 36) - 1),
                        md5=bytes(body[18:34]))
        elif kind == SEEKTABLE:
            points = parse_seektable(bytes(body))
        pos += 4 + size
        if head & 0x80:
            break
    if info is None:
        raise ValueError("no STREAMINFO block")
    return info, points, pos
