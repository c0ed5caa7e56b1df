"""The DAB+ superframe reader in plain Python (include/dabgpu.h, "the superframe reader"; ETSI TS 102 563 5.2-5.4, 6): the oracle
of tests/test_superframe_*.py.  GF(2^8) with x^8 + x^4 + x^3 + x^2 + 1, RS(120,110) shortened from RS(255,245) with
g(x) = prod_{i = 0 ... 9} (x + alpha^i), encoder and decoder (syndromes, Berlekamp-Massey, Chien search over the 120 real positions,
Forney; a word whose locator has a root outside them is uncorrectable), Fire code, header, AU CRC, the record of one candidate,
the greedy walk over a call's records, and a builder of superframes.  All integers."""
import struct

import numpy as np

N, K, T2, PAD = 120, 110, 10, 135
FIRE_OK, ZERO, HEADER_VALID, RS_FAILED = 1, 2, 4, 8
RECORD_BYTES = 64
FAILED = 0xFF

EXP = [0] * 512
LOG = [0] * 256
_x = 1
for _i in range(255):
    EXP[_i] = _x
    LOG[_x] = _i
    _x <<= 1
    if _x & 0x100:
        _x ^= 0x11D
for _i in range(255, 512):
    EXP[_i] = EXP[_i - 255]


def mul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def inv(a):
    return EXP[255 - LOG[a]]


def _generator():
    g = [1]                                               # lowest degree first
    for i in range(T2):
        g = [(g[k - 1] if k else 0) ^ (mul(g[k], EXP[i]) if k < len(g) else 0) for k in range(len(g) + 1)]
    return g


GEN = _generator()


def rs_parity(data):
    """the ten parity bytes behind 110 data bytes: the remainder of data(x) x^10 by g(x), highest degree first"""
    assert len(data) == K
    reg = [0] * T2                                        # reg[0]: highest degree
    for d in data:
        fb = d ^ reg[0]
        reg = [reg[k + 1] ^ mul(fb, GEN[T2 - 1 - k]) for k in range(T2 - 1)] + [mul(fb, GEN[0])]
    return bytes(reg)


def rs_encode(data):
    return bytes(data) + rs_parity(data)


def rs_syndromes(word):
    """S_j = sum_p word[p] alpha^(j (119 - p)), j = 0 ... 9"""
    s = [0] * T2
    for j in range(T2):
        acc = 0
        for b in word:
            acc = mul(acc, EXP[j]) ^ b
        s[j] = acc
    return s


def rs_decode(word):
    """(corrected word, count): count = bytes corrected, -1 = uncorrectable (the word comes back untouched).  Berlekamp-Massey
    as libfec runs it; the Chien search looks at the 120 real positions only and the word is refused unless every root of the
    locator is among them."""
    word = bytes(word)
    assert len(word) == N
    s = rs_syndromes(word)
    if not any(s):
        return word, 0
    lam = [1] + [0] * T2
    b = [1] + [0] * T2
    el = 0
    for r in range(1, T2 + 1):
        d = 0
        for i in range(r):
            d ^= mul(lam[i], s[r - 1 - i])
        if d == 0:
            b = [0] + b[:T2]
            continue
        t = [lam[0]] + [lam[i + 1] ^ mul(d, b[i]) for i in range(T2)]
        if 2 * el <= r - 1:
            el = r - el
            di = inv(d)
            b = [mul(x, di) for x in lam]
        else:
            b = [0] + b[:T2]
        lam = t
    deg = max(i for i in range(T2 + 1) if lam[i])
    roots = []                                            # (position, z): lambda(alpha^z) = 0, z = 136 + position
    for p in range(N):
        z = (136 + p) % 255
        q = 0
        for j in range(T2 + 1):
            if lam[j]:
                q ^= EXP[(LOG[lam[j]] + j * z) % 255]
        if q == 0:
            roots.append((p, z))
    if len(roots) != deg:
        return word, -1
    omega = [0] * T2
    for i in range(deg):
        for j in range(i + 1):
            omega[i] ^= mul(s[i - j], lam[j])
    out = bytearray(word)
    for p, z in roots:
        num1 = 0
        for i in range(deg):
            if omega[i]:
                num1 ^= EXP[(LOG[omega[i]] + i * z) % 255]
        num2 = EXP[(255 - z) % 255]
        den = 0
        for i in range(0, min(deg, T2 - 1) + 1, 2):
            if lam[i + 1]:
                den ^= EXP[(LOG[lam[i + 1]] + i * z) % 255]
        assert den, "a simple root has a non-zero derivative"
        out[p] ^= mul(mul(num1, num2), inv(den))
    return bytes(out), deg


def crc16(data, poly, init):
    crc = init
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ poly if crc & 0x8000 else crc << 1) & 0xFFFF
    return crc


def fire_crc(header9):
    """the Fire code word of bytes 2 ... 10"""
    return crc16(header9, 0x782F, 0)


def au_crc(data):
    return crc16(data, 0x1021, 0xFFFF) ^ 0xFFFF


AU_TABLE = {(0, 1): (2, 5), (1, 1): (3, 6), (0, 0): (4, 8), (1, 0): (6, 11)}


def parse_header(sf, s):
    """the header fields of a superframe's corrected bytes: dict of header (byte 2), rfa ... mpeg_surround_config, num_aus,
    au_start (7 entries, zero behind num_aus + 1) and valid"""
    h = sf[2]
    d = dict(header=h, rfa=h >> 7, dac_rate=(h >> 6) & 1, sbr_flag=(h >> 5) & 1, aac_channel_mode=(h >> 4) & 1, ps_flag=(h >> 3) & 1,
             mpeg_surround_config=h & 7)
    num, first = AU_TABLE[(d["dac_rate"], d["sbr_flag"])]
    start = [first]
    for k in range(num - 1):
        bit = 24 + 12 * k
        byte = bit // 8
        v = sf[byte] << 8 | sf[byte + 1]
        start.append((v >> 4) if bit % 8 == 0 else (v & 0xFFF))
    start.append(K * s)
    d["num_aus"] = num
    d["valid"] = all(start[k + 1] - start[k] >= 3 for k in range(num))
    d["au_start"] = start + [0] * (7 - len(start))
    return d


def candidate(frames, s):
    """one candidate: the 120 s bytes of five sub-channel frames -> (record dict, 110 s output bytes)"""
    buf = bytes(frames)
    assert len(buf) == N * s
    out = bytearray(K * s)
    cw = [0] * 24
    for i in range(s):
        word, n = rs_decode(buf[i::s])
        cw[i] = FAILED if n < 0 else n
        out[i::s] = word[:K]
    good = [c for c in cw[:s] if c != FAILED]
    rec = dict(flags=0, rs_corrected=sum(good), rs_failed=s - len(good), rs_max=max(good + [0]), cw_errors=cw, au_ok=0)
    rec["fire_crc"] = fire_crc(out[2:11])
    if rec["rs_failed"]:
        rec["flags"] |= RS_FAILED
    if rec["fire_crc"] == (out[0] << 8 | out[1]):
        rec["flags"] |= FIRE_OK
    if not any(out[:11]):
        rec["flags"] |= ZERO
    rec.update(parse_header(out, s))
    if rec.pop("valid"):
        rec["flags"] |= HEADER_VALID
    if accepted(rec):
        for k in range(rec["num_aus"]):
            a, b = rec["au_start"][k], rec["au_start"][k + 1]
            if au_crc(out[a:b - 2]) == (out[b - 2] << 8 | out[b - 1]):
                rec["au_ok"] |= 1 << k
    return rec, bytes(out)


def accepted(rec):
    return rec["flags"] & (FIRE_OK | ZERO | HEADER_VALID) == (FIRE_OK | HEADER_VALID)


def pack_record(r):
    """the 64 bytes of dabgpu_sf_record"""
    b = struct.pack("<IHHBBBB6B2x7HH", r["flags"], r["rs_corrected"], r["rs_failed"], r["rs_max"], r["num_aus"], r["au_ok"], r["header"],
                    r["rfa"], r["dac_rate"], r["sbr_flag"], r["aac_channel_mode"], r["ps_flag"], r["mpeg_surround_config"],
                    *r["au_start"], r["fire_crc"]) + bytes(r["cw_errors"]) + bytes(4)
    assert len(b) == RECORD_BYTES
    return b


def unpack_record(b):
    b = bytes(b)
    v = struct.unpack("<IHHBBBB6B2x7HH", b[:36])
    keys = ("flags", "rs_corrected", "rs_failed", "rs_max", "num_aus", "au_ok", "header", "rfa", "dac_rate", "sbr_flag", "aac_channel_mode",
            "ps_flag", "mpeg_surround_config")
    r = dict(zip(keys, v[:13]))
    r["au_start"] = list(v[13:20])
    r["fire_crc"] = v[20]
    r["cw_errors"] = list(b[36:60])
    return r


def scan(images, offset, framesize):
    """what one call gives: (records, output bytes) of the n - 4 candidates of (n, 6144) uint8 images"""
    images = np.asarray(images, np.uint8).reshape(-1, 6144)
    s = framesize // 24
    sub = images[:, offset:offset + framesize]
    recs, out = [], []
    for f in range(images.shape[0] - 4):
        r, o = candidate(sub[f:f + 5].tobytes(), s)
        recs.append(r)
        out.append(o)
    return recs, b"".join(out)


def walk(recs):
    """the greedy walk over a call's records: dabgpu_sf_result as a dict; `accepted`: the indices"""
    res = dict(candidates=len(recs), superframes=0, first=-1, phase_changes=0, aus=0, aus_ok=0, aus_bad=0, rs_corrected=0, rs_failed=0,
               rs_max=0, accepted=[])
    f, last = 0, None
    while f < len(recs):
        r = recs[f]
        if not accepted(r):
            f += 1
            continue
        if last is None:
            res["first"] = f
        elif f % 5 != last % 5:
            res["phase_changes"] += 1
        last = f
        ok = bin(r["au_ok"]).count("1")
        res["superframes"] += 1
        res["aus"] += r["num_aus"]
        res["aus_ok"] += ok
        res["aus_bad"] += r["num_aus"] - ok
        res["rs_corrected"] += r["rs_corrected"]
        res["rs_failed"] += r["rs_failed"]
        res["rs_max"] = max(res["rs_max"], r["rs_max"])
        res["accepted"].append(f)
        f += 5
    return res


def slice_aus(out, res, recs, s):
    """the AUs of the accepted superframes, without their CRCs: ([bytes], [crc ok])"""
    aus, ok = [], []
    for f in res["accepted"]:
        sf = out[f * K * s:(f + 1) * K * s]
        r = recs[f]
        for k in range(r["num_aus"]):
            aus.append(bytes(sf[r["au_start"][k]:r["au_start"][k + 1] - 2]))
            ok.append(bool(r["au_ok"] >> k & 1))
    return aus, ok


# ---- the builder
def build_superframe(s, rs, dac_rate=1, sbr_flag=0, channel_mode=1, ps_flag=0, surround=0, sizes=None):
    """(the 120 s bytes of one superframe, its AUs' payload): random AUs of about equal size (or of `sizes`, CRC included), header,
    Fire code, AU CRCs, RS parity"""
    num, first = AU_TABLE[(dac_rate, sbr_flag)]
    total = K * s - first
    if sizes is None:
        sizes = [total // num] * num
        sizes[-1] += total - sum(sizes)
    assert len(sizes) == num and sum(sizes) == total and min(sizes) >= 3
    sf = bytearray(K * s)
    sf[2] = dac_rate << 6 | sbr_flag << 5 | channel_mode << 4 | ps_flag << 3 | surround
    start = [first]
    for z in sizes[:-1]:
        start.append(start[-1] + z)
    bits = 0
    nbits = 0
    for v in start[1:]:
        bits = bits << 12 | v
        nbits += 12
    if nbits % 8:
        bits <<= 4
        nbits += 4
    sf[3:3 + nbits // 8] = bits.to_bytes(nbits // 8, "big")
    aus = []
    for a, z in zip(start, sizes):
        au = bytes(rs.randint(0, 256, z - 2).astype(np.uint8))
        c = au_crc(au)
        sf[a:a + z] = au + bytes([c >> 8, c & 0xFF])
        aus.append(au)
    c = fire_crc(sf[2:11])                                # (bytes 2 ... 10: with two, three or four AUs the first one's bytes are among them)
    sf[0], sf[1] = c >> 8, c & 0xFF
    return rs_protect(bytes(sf), s), aus


def rs_protect(data, s):
    """110 s data bytes -> 120 s bytes: codeword i is bytes i, i + s, ..."""
    assert len(data) == K * s
    out = bytearray(N * s)
    for i in range(s):
        out[i::s] = rs_encode(data[i::s])
    return bytes(out)


def stream_images(n_images, s, offset, phase, seed, fill="random", **kw):
    """(images (n, 6144) uint8, [(first image, AUs)]): superframes from image `phase` on, five images each, while they fit whole;
    `fill` outside the sub-channel (and in the sub-channel where no superframe lies): random bytes or zero"""
    rs = np.random.RandomState(seed)
    images = rs.randint(0, 256, (n_images, 6144)).astype(np.uint8) if fill == "random" else np.zeros((n_images, 6144), np.uint8)
    fs = 24 * s
    placed = []
    f = phase
    while f + 5 <= n_images:
        sf, aus = build_superframe(s, rs, **kw)
        images[f:f + 5, offset:offset + fs] = np.frombuffer(sf, np.uint8).reshape(5, fs)
        placed.append((f, aus))
        f += 5
    return images, placed
