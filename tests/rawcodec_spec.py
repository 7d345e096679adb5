"""The raw codec "TDKR" (include/tdk_hip_rawcodec.h, the normative text) restated in NumPy: `encode` / `decode` vectorised, as the tests
of the device kernels use them, and `encode_loops` / `decode_loops` as literal per-sample loops that hold the vectorised forms on small
frames.  Also the frames the tests share, the packed 12-bit forms and the float conversions of the decoder's outputs."""

import struct

import numpy as np

MAGIC, VERSION, HEADER_BYTES = b'TDKR', 1, 32
SPAN, SEGMENT = 64, 512
ROWS = 256   # rows the vectorised forms take at a time
BAD_MAGIC, BAD_SIZE, BAD_TABLES = 1, 2, 4
PACKED12, PACKED12_IDS, U16, F32, F16 = 0, 1, 2, 3, 4   # the TDK_RAW_* values of include/tdk_hip_raw.h


def geometry(width, height):
    """(S, G): spans and segments of a row."""
    assert 1 <= width <= 65535 and 1 <= height <= 65535 and width * height <= 1 << 30
    return -(-width // SPAN), -(-width // SEGMENT)


def round4(n):
    return (n + 3) // 4 * 4


def table_bytes(width, height):
    s, g = geometry(width, height)
    return HEADER_BYTES + 8 * height * g + round4(2 * height * s)


def max_stream_bytes(width, height):
    s, _ = geometry(width, height)
    return table_bytes(width, height) + 4 * 16 * 2 * height * s


def sections(width, height):
    """Byte offsets of anchors, offsets, widths and payload."""
    s, g = geometry(width, height)
    anchors = HEADER_BYTES
    offsets = anchors + 4 * height * g
    widths = offsets + 4 * height * g
    return anchors, offsets, widths, widths + round4(2 * height * s)


def header(width, height, bits, payload_words):
    return MAGIC + struct.pack('<HHIIIIII', VERSION, bits, width, height, payload_words, table_bytes(width, height) + 4 * payload_words, 0, 0)


def parse_header(data):
    """(version, bits, width, height, payload_words, total_bytes, flags, reserved) of a stream whose magic is right."""
    raw = bytes(np.asarray(data, dtype=np.uint8)[:HEADER_BYTES])
    assert raw[:4] == MAGIC
    return struct.unpack('<HHIIIIII', raw[4:])


def zigzag(d):
    """d: differences mod 2^16 as integers 0..65535."""
    d = np.asarray(d, dtype=np.int64) & 0xFFFF
    t = np.where(d >= 0x8000, d - 0x10000, d)
    return ((t << 1) ^ (t >> 15)) & 0xFFFF


def unzigzag(z):
    z = np.asarray(z, dtype=np.int64)
    return ((z >> 1) ^ -(z & 1)) & 0xFFFF


def bit_length(v):
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros(v.shape, dtype=np.int64)
    for j in range(16):
        out = np.where(v >> j, j + 1, out)
    return out


# ---- vectorised

def _chains(frame):
    """(H, G, 256, 2) int64: the sequences v_k of every segment and parity, zero where the site does not exist, and that mask."""
    h, w = frame.shape
    _, g = geometry(w, h)
    padded = np.zeros((h, g * SEGMENT), dtype=np.int64)
    padded[:, :w] = frame
    exists = np.zeros((h, g * SEGMENT), dtype=bool)
    exists[:, :w] = True
    return padded.reshape(h, g, SEGMENT // 2, 2), exists.reshape(h, g, SEGMENT // 2, 2)


def encode(frame, bits=12):
    """(H, W) uint16 -> the stream, a uint8 array of total_bytes."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint16 and frame.ndim == 2 and 1 <= bits <= 16
    h, w = frame.shape
    s, g = geometry(w, h)
    v, exists = _chains(frame)
    d = np.zeros_like(v)
    d[:, :, 1:] = v[:, :, 1:] - v[:, :, :-1]
    z = np.where(exists, zigzag(d), 0)
    groups = z.reshape(h, g * 8, 32, 2)[:, :s].transpose(0, 1, 3, 2)              # [y, span, parity, sample], the spans that exist
    b = bit_length(groups.max(axis=-1))                                           # [y, span, parity]
    payload = []
    for r in range(0, h, ROWS):   # (some rows at a time: the planes of a tall frame are sixteen times its size)
        planes = (((groups[r:r + ROWS, ..., None, :] >> np.arange(16)[:, None]) & 1) << np.arange(32)).sum(axis=-1)   # [y, span, parity, plane]
        payload.append(planes[np.arange(16) < b[r:r + ROWS, ..., None]].astype('<u4'))   # row-major: y, span, parity, plane
    payload = np.concatenate(payload)
    padded = np.zeros((h, g * 8, 2), dtype=np.int64)
    padded[:, :s] = b
    counts = padded.reshape(h, g, 16).sum(axis=-1).reshape(-1)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype('<u4')
    widths = np.zeros(round4(2 * h * s), dtype=np.uint8)
    widths[:2 * h * s] = b.reshape(-1)
    anchors = v[:, :, 0, :].astype('<u2')
    parts = [np.frombuffer(header(w, h, bits, payload.size), dtype=np.uint8), anchors.reshape(-1).view(np.uint8), offsets.view(np.uint8), widths,
             payload.reshape(-1).view(np.uint8)]
    out = np.concatenate(parts)
    assert out.size == table_bytes(w, h) + 4 * payload.size
    return out


def decode(data, width, height):
    """The stream (uint8, its whole length counts as data_bytes) -> ((H, W) uint16, status), as tdk_rawcodec_decode does."""
    data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    assert data.size >= HEADER_BYTES
    s, g = geometry(width, height)
    zero = np.zeros((height, width), dtype=np.uint16)
    version, _, w, h = struct.unpack('<HHII', bytes(data[4:16]))
    status = (BAD_MAGIC if bytes(data[:4]) != MAGIC or version != VERSION else 0) | (BAD_SIZE if (w, h) != (width, height) else 0)
    if status:
        return zero, status
    if table_bytes(width, height) > data.size:
        return zero, BAD_TABLES
    at_anchors, at_offsets, at_widths, at_payload = sections(width, height)
    anchors = data[at_anchors:at_offsets].view('<u2').astype(np.int64).reshape(height, g, 1, 2)
    offsets = data[at_offsets:at_widths].view('<u4').astype(np.int64).reshape(height, g)
    b = np.zeros((height, g * 8, 2), dtype=np.int64)
    b[:, :s] = data[at_widths:at_widths + 2 * height * s].reshape(height, s, 2)
    per_segment = b.reshape(height, g, 16)                                          # [y, g, group]: span * 2 + parity
    bad = (per_segment > 16).any(axis=-1) | (at_payload + 4 * (offsets + per_segment.sum(axis=-1)) > data.size)
    words = data[at_payload:at_payload + (data.size - at_payload) // 4 * 4].view('<u4').astype(np.int64)
    starts = offsets[..., None] + np.cumsum(per_segment, axis=-1) - per_segment
    live = 2 * s                                                                    # the groups of a row that exist
    width_of = per_segment.reshape(height, g * 16)[:, :live]
    starts = starts.reshape(height, g * 16)[:, :live]
    good = np.repeat(~bad, 16, axis=1)[:, :live]
    index = starts[..., None] + np.arange(16)                                       # [y, group, plane]
    used = (np.arange(16) < width_of[..., None]) & good[..., None]
    plane_words = np.where(used, np.concatenate([words, [0]])[np.where(used, index, words.size)], 0)
    z = np.concatenate([(((plane_words[r:r + ROWS, ..., None] >> np.arange(32)) & 1) << np.arange(16)[:, None]).sum(axis=-2)
                        for r in range(0, height, ROWS)])                           # [y, group, sample]
    t = np.zeros((height, g * 8, 32, 2), dtype=np.int64)
    t[:, :s] = unzigzag(z).reshape(height, s, 2, 32).transpose(0, 1, 3, 2)
    t = t.reshape(height, g, SEGMENT // 2, 2)
    t[:, :, 0] = 0                                                                  # the chain's first sample is its anchor
    v = (anchors + np.cumsum(t, axis=2)) & 0xFFFF
    v = np.where(bad[..., None, None], 0, v)
    out = v.reshape(height, g * SEGMENT)[:, :width].astype(np.uint16)
    return out, (BAD_TABLES if bad.any() else 0)


# ---- literal loops (small frames)

def encode_loops(frame, bits=12):
    frame = np.asarray(frame)
    h, w = frame.shape
    s, g = geometry(w, h)
    anchors, widths, payload, offsets = [], [], [], []
    for y in range(h):
        row_widths = {}
        for seg in range(g):
            offsets.append(len(payload))
            z_of = {}
            for p in (0, 1):
                chain = [int(frame[y, x]) for x in range(SEGMENT * seg + p, min(w, SEGMENT * (seg + 1)), 2)]
                anchors.append(chain[0] if chain else 0)
                for k, value in enumerate(chain):
                    d = 0 if k == 0 else (value - chain[k - 1]) % 65536
                    t = d - 65536 if d >= 32768 else d
                    z_of[SEGMENT * seg + 2 * k + p] = ((t << 1) ^ (t >> 15)) & 0xFFFF
            for span in range(8 * seg, min(s, 8 * (seg + 1))):
                for p in (0, 1):
                    zs = [z_of.get(SPAN * span + 2 * i + p, 0) for i in range(32)]
                    b = max(zs).bit_length()
                    row_widths[(span, p)] = b
                    for j in range(b):
                        payload.append(sum(((zs[i] >> j) & 1) << i for i in range(32)))
        widths += [row_widths[(span, p)] for span in range(s) for p in (0, 1)]
    widths += [0] * (round4(len(widths)) - len(widths))
    out = header(w, h, bits, len(payload)) + b''.join(struct.pack('<H', a) for a in anchors) + b''.join(struct.pack('<I', o) for o in offsets)
    out += bytes(widths) + b''.join(struct.pack('<I', word) for word in payload)
    return np.frombuffer(out, dtype=np.uint8).copy()


def decode_loops(data, width, height):
    """A valid stream only."""
    raw = bytes(np.asarray(data, dtype=np.uint8))
    s, g = geometry(width, height)
    at_anchors, at_offsets, at_widths, at_payload = sections(width, height)
    out = np.zeros((height, width), dtype=np.uint16)
    for y in range(height):
        for seg in range(g):
            n = y * g + seg
            at = struct.unpack_from('<I', raw, at_offsets + 4 * n)[0]
            value = list(struct.unpack_from('<HH', raw, at_anchors + 4 * n))
            for span in range(8 * seg, min(s, 8 * (seg + 1))):
                zs = {}
                for p in (0, 1):
                    b = raw[at_widths + 2 * (y * s + span) + p]
                    words = struct.unpack_from(f'<{b}I', raw, at_payload + 4 * at)
                    at += b
                    zs[p] = [sum(((words[j] >> i) & 1) << j for j in range(b)) for i in range(32)]
                for i in range(32):
                    for p in (0, 1):
                        x = SPAN * span + 2 * i + p
                        if x < width:
                            z = zs[p][i]
                            value[p] = (value[p] + ((z >> 1) ^ -(z & 1))) % 65536
                            out[y, x] = value[p]
    return out


# ---- the other forms of a frame

def pack12(samples, ids=False):
    """The bytes tdk_decode12_u16 reads the samples from, saturated at 4095: those of tdk_encode12_u16 for the standard order; for the
    IDS order the inverse of the decoder (tdk_encode12_u16 puts the two low nibbles the other way round than tdk_decode12_u16 reads them)."""
    flat = np.minimum(np.asarray(samples).reshape(-1).astype(np.int64), 4095)
    assert flat.size % 2 == 0
    p0, p1 = flat[0::2], flat[1::2]
    if ids:
        triples = (p0 >> 4, p1 >> 4, ((p1 & 15) << 4) | (p0 & 15))
    else:
        triples = (p0 & 255, ((p1 & 15) << 4) | (p0 >> 8), p1 >> 4)
    return np.stack(triples, axis=1).reshape(-1).astype(np.uint8)


def unpack12(packed, ids=False):
    """The samples of tdk_decode12_u16, flat."""
    b = np.asarray(packed, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    if ids:
        p0, p1 = (b[:, 0] << 4) | (b[:, 2] & 15), (b[:, 1] << 4) | (b[:, 2] >> 4)
    else:
        p0, p1 = ((b[:, 1] & 15) << 8) | b[:, 0], (b[:, 2] << 4) | (b[:, 1] >> 4)
    return np.stack((p0, p1), axis=1).reshape(-1).astype(np.uint16)


def to_float32(samples):
    """The bits of tdk_decode12_f32 with scaled on: one float32 product."""
    return np.asarray(samples).astype(np.float32) * np.float32(1.0 / 4095.0)


def to_float16(samples):
    return to_float32(samples).astype(np.float16)


# ---- the frames the tests share; every one is a pure function of (class, width, height)

CLASSES = ('constant', 'uniform', 'alternating', 'wrap', 'ramp', 'outlier')


def noisy_ramp(width, height, a=1e-4, b=4e-6, seed=12):
    """A 12-bit ramp along the row with Poisson-Gaussian noise of variance a*s + b on the signal s in 0..1."""
    rng = np.random.default_rng(seed)
    s = np.broadcast_to(np.linspace(0.02, 0.9, width), (height, width))
    noisy = s + np.sqrt(a * s + b) * rng.standard_normal((height, width))
    return np.clip(np.rint(noisy * 4095.0), 0, 4095).astype(np.uint16)


def frame(kind, width, height):
    rng = np.random.default_rng(1000 * CLASSES.index(kind) + 7 * width + height)
    x = np.broadcast_to(np.arange(width), (height, width))
    if kind == 'constant':
        return np.full((height, width), 1234, dtype=np.uint16)
    if kind == 'uniform':
        return rng.integers(0, 65536, (height, width)).astype(np.uint16)
    if kind == 'alternating':   # same-parity samples alternate 0 and 0x8000: every difference is -32768, z = 0xFFFF
        return np.where((x // 2) % 2 == 1, 0x8000, 0).astype(np.uint16)
    if kind == 'wrap':          # 0 and 65535: differences of +-1 through the wrap-around
        return np.where((x // 2 + np.arange(height)[:, None]) % 2 == 1, 65535, 0).astype(np.uint16)
    if kind == 'ramp':
        return noisy_ramp(width, height, seed=width + height)
    if kind == 'outlier':       # quiet 12-bit data, one sample far off in every group of 32 same-parity sites
        base = (2000 + rng.integers(-3, 4, (height, width))).astype(np.int64)
        group = x // SPAN * 2 + x % 2
        hit = (x % SPAN) // 2 == (5 * group + 3) % 32
        return np.where(hit, rng.integers(0, 65536, (height, width)), base).astype(np.uint16)
    raise ValueError(kind)


def as_12bit(samples):
    """A frame a packed container can hold: the low 12 bits."""
    return (np.asarray(samples) & 0x0FFF).astype(np.uint16)
