"""Host model of the handle snapshot format (csrc/sechs_snapshot.h owns it; sn_state_save / sn_state_load).

A snapshot is one uint8 blob: a 320-byte header, then one fixed-size record per game, game-major.  `layout` gives
the dword offsets of a record, `unpack_host` / `pack_host` turn a blob into numpy arrays and back, and
`mt_canonical_host` is the conversion k_snapshot_save performs on the device: the library's lazy MT19937 form
(the raw 624 words, the state code, the newest old mt[0]) to np.random.get_state()'s (key, pos).  Records carry
that canonical form, so `np.random.RandomState().set_state(("MT19937", key, pos))` continues a game's stream.

No GPU and no library call here: tests/test_snapshot_cpu.py holds this model against sn_state_bytes."""
import numpy as np

MAGIC, VERSION, HEADER_BYTES = 0x50534E53, 1, 320
RNG_PHILOX, RNG_NUMPY_MT = 0, 1
MT_N, MT_M = 624, 397
_MATRIX_A, _UPPER, _LOWER = 0x9908B0DF, 0x80000000, 0x7FFFFFFF

# the header as a numpy record (SnapHeader)
HEADER_DTYPE = np.dtype([
    ("magic", "<u4"), ("version", "<u4"), ("header_bytes", "<u4"), ("record_bytes", "<u4"),
    ("B", "<i8"), ("N", "<i4"), ("C", "<i4"), ("rng_mode", "<i4"), ("league", "<i4"),
    ("seed", "<u8"), ("game_offset", "<u8"),
    ("lg_K", "<i4"), ("lg_lo", "<i4"), ("lg_hi", "<i4"), ("phase", "<i4"), ("lg_phase", "<i4"), ("overruns", "<u4"),
    ("lg_kind", "<i4", (16,)), ("lg_mpc", "<i4", (16,)), ("lg_mmax", "<i4", (16,)), ("pad1", "<u4", (12,)),
])
assert HEADER_DTYPE.itemsize == HEADER_BYTES


def layout(num_players, rng_mode, league=False):
    """dword offsets of a record's fields (snap_layout): hand, row_lo, row_hi, score, sum_res, episodes, lgs and
    lmem (tournament handles; else -1), then pos / key (numpy-MT) or ctr (Philox); `dwords` = the record size,
    `record_bytes` = 4 * dwords, a multiple of 16"""
    N, o = int(num_players), 0
    L = {}
    for name, n in (("hand", 3 * N), ("row_lo", 4), ("row_hi", 4), ("score", N), ("sum_res", N), ("episodes", 1)):
        L[name], o = o, o + n
    L["lgs"] = L["lmem"] = -1
    if league:
        L["lgs"], o = o, o + 1
        L["lmem"], o = o, o + 4 * N
    L["small"] = o
    L["pos"] = L["key"] = L["ctr"] = -1
    if rng_mode == RNG_NUMPY_MT:
        L["key"] = (o + 1 + 3) & ~3
        L["pos"] = L["key"] - 1
        o = L["key"] + MT_N
    else:
        L["ctr"] = (o + 1) & ~1
        o = L["ctr"] + 2
    L["dwords"] = (o + 3) & ~3
    L["record_bytes"] = 4 * L["dwords"]
    L["header_bytes"] = HEADER_BYTES
    return L


def state_bytes(num_games, num_players, rng_mode, league=False):
    """the blob size sn_state_bytes answers"""
    return HEADER_BYTES + int(num_games) * layout(num_players, rng_mode, league)["record_bytes"]


def read_header(blob):
    """the header of a blob (uint8 numpy array or anything np.asarray takes) as a dict of Python values"""
    raw = np.ascontiguousarray(np.asarray(blob, dtype=np.uint8)[:HEADER_BYTES])
    if raw.size < HEADER_BYTES:
        raise ValueError("the blob is shorter than a snapshot header")
    h = raw.view(HEADER_DTYPE)[0]
    return {k: (h[k].copy() if h[k].shape else h[k].item()) for k in HEADER_DTYPE.names if not k.startswith("pad")}


def unpack_host(blob):
    """blob -> (header dict, fields dict of numpy arrays over the blob's B games): hand [B, N, 3] uint32, row_lo /
    row_hi [B, 4] uint32, score / sum_res [B, N] int32, episodes [B] int32, lgs [B] uint32 and lmem [B, N, 4]
    uint32 (tournament snapshots), pos [B] int32 and key [B, 624] uint32 (numpy-MT) or ctr [B] uint64 (Philox)"""
    blob = np.ascontiguousarray(np.asarray(blob, dtype=np.uint8))
    h = read_header(blob)
    if h["magic"] != MAGIC or h["version"] != VERSION:
        raise ValueError("not a snapshot of this format version")
    B, N = h["B"], h["N"]
    L = layout(N, h["rng_mode"], bool(h["league"]))
    if h["record_bytes"] != L["record_bytes"] or blob.size < HEADER_BYTES + B * L["record_bytes"]:
        raise ValueError("the blob does not hold the records its header names")
    rec = blob[HEADER_BYTES: HEADER_BYTES + B * L["record_bytes"]].view("<u4").reshape(B, L["dwords"])
    f = {
        "hand": rec[:, L["hand"]: L["hand"] + 3 * N].reshape(B, N, 3).copy(),
        "row_lo": rec[:, L["row_lo"]: L["row_lo"] + 4].copy(),
        "row_hi": rec[:, L["row_hi"]: L["row_hi"] + 4].copy(),
        "score": rec[:, L["score"]: L["score"] + N].astype(np.int32),
        "sum_res": rec[:, L["sum_res"]: L["sum_res"] + N].astype(np.int32),
        "episodes": rec[:, L["episodes"]].astype(np.int32),
    }
    if h["league"]:
        f["lgs"] = rec[:, L["lgs"]].copy()
        f["lmem"] = rec[:, L["lmem"]: L["lmem"] + 4 * N].reshape(B, N, 4).copy()
    if h["rng_mode"] == RNG_NUMPY_MT:
        f["pos"] = rec[:, L["pos"]].astype(np.int32)
        f["key"] = rec[:, L["key"]: L["key"] + MT_N].copy()
    else:
        c = rec[:, L["ctr"]: L["ctr"] + 2].astype(np.uint64)
        f["ctr"] = c[:, 0] | (c[:, 1] << np.uint64(32))
    return h, f


def pack_host(header, fields):
    """the inverse of unpack_host: a uint8 blob (padding zero, as k_snapshot_save writes it)"""
    B, N = int(header["B"]), int(header["N"])
    L = layout(N, header["rng_mode"], bool(header["league"]))
    hdr = np.zeros(1, dtype=HEADER_DTYPE)
    for k, v in header.items():
        hdr[k][0] = v
    hdr["magic"], hdr["version"], hdr["header_bytes"], hdr["record_bytes"] = MAGIC, VERSION, HEADER_BYTES, L["record_bytes"]
    rec = np.zeros((B, L["dwords"]), dtype="<u4")
    rec[:, L["hand"]: L["hand"] + 3 * N] = np.asarray(fields["hand"], dtype=np.uint32).reshape(B, 3 * N)
    rec[:, L["row_lo"]: L["row_lo"] + 4] = fields["row_lo"]
    rec[:, L["row_hi"]: L["row_hi"] + 4] = fields["row_hi"]
    rec[:, L["score"]: L["score"] + N] = np.asarray(fields["score"], dtype=np.int32).view(np.uint32)
    rec[:, L["sum_res"]: L["sum_res"] + N] = np.asarray(fields["sum_res"], dtype=np.int32).view(np.uint32)
    rec[:, L["episodes"]] = np.asarray(fields["episodes"], dtype=np.int32).view(np.uint32)
    if header["league"]:
        rec[:, L["lgs"]] = fields["lgs"]
        rec[:, L["lmem"]: L["lmem"] + 4 * N] = np.asarray(fields["lmem"], dtype=np.uint32).reshape(B, 4 * N)
    if header["rng_mode"] == RNG_NUMPY_MT:
        rec[:, L["pos"]] = np.asarray(fields["pos"], dtype=np.int32).view(np.uint32)
        rec[:, L["key"]: L["key"] + MT_N] = fields["key"]
    else:
        c = np.asarray(fields["ctr"], dtype=np.uint64)
        rec[:, L["ctr"]] = (c & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        rec[:, L["ctr"] + 1] = (c >> np.uint64(32)).astype(np.uint32)
    return np.concatenate((hdr.view(np.uint8).reshape(-1), rec.view(np.uint8).reshape(-1)))


# ---------------------------------------------------------------- the MT19937 state, lazy form -> numpy form
def _mix(a, b, c):
    y = (a & _UPPER) | (b & _LOWER)
    return c ^ (y >> 1) ^ (_MATRIX_A if y & 1 else 0)


def _untwist_y(t):
    lsb = t >> 31
    if lsb:
        t ^= _MATRIX_A
    return ((t << 1) & 0xFFFFFFFF) | lsb


def mt_canonical_host(raw_key, code, old0=0):
    """(key uint32 [624], pos) in np.random.get_state() form of the lazy state (raw_key, code, old0).

    code = p | cnt << 16 (csrc/sechs_device.h, at MtGenT): words [0, p) of raw_key hold this round's values,
    [p, 624) the round's before; cnt words just before p are twisted and not consumed yet.
      p == 0 or p == 624   a complete round (code 0: np.random.seed's state, pos 624): copied;
      0 < p < 624, cnt < p   mid-round: words [p, 624) are twisted in place, pos = p - cnt;
      cnt > p > 0   straddled: the consumer is still in the round before, whose head [0, p) the twist has
                    overwritten; it is untwisted (old0: the old mt[0], whose low 31 bits the twist never
                    reads), pos = 624 + p - cnt;
      cnt == p < 624   straddled as well: the consumer has drawn its round's last word, and numpy, which
                    twists at the next draw, shows that round at pos 624.  cnt == p == 624 is the import of
                    numpy's pos 0 (mt_code_from_numpy) and stays pos 0 (mt_code_straddles, csrc/sechs_device.h)."""
    a = [int(x) for x in np.asarray(raw_key, dtype=np.uint32)]
    assert len(a) == MT_N
    p, cnt = int(code) & 0x7FF, (int(code) >> 16) & 0x3FF
    D = MT_N - MT_M
    straddles = p > 0 and (cnt > p or (cnt == p and p < MT_N))
    if straddles:
        y = [0] * MT_N
        for j in range(D, p):
            y[j] = _untwist_y(a[j] ^ a[j - D])

        def old_at(m):  # m >= 397
            return ((y[m] & _UPPER) | (y[m - 1] & _LOWER)) if m < p else a[m]

        for j in range(0, min(p, D)):
            y[j] = _untwist_y(a[j] ^ old_at(j + MT_M))
        for j in range(p):
            a[j] = (y[j] & _UPPER) | ((int(old0) if j == 0 else y[j - 1]) & _LOWER)
    elif 0 < p < MT_N:
        for i in range(p, MT_N):
            a[i] = _mix(a[i], a[(i + 1) % MT_N], a[(i + MT_M) % MT_N])
    if p == 0:
        pos = MT_N
    else:
        pos = MT_N + p - cnt if straddles else p - cnt
    return np.array(a, dtype=np.uint32), pos
