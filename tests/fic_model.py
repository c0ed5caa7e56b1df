"""A plain-Python model of the FIC reader (include/dabgpu.h, "the FIC reader"; odr-dabmod_amd/csrc/fic.hip, api_fic.hip), written
from EN 300 401 5.2 (FIB, CRC, FIG header), 6.2.1 (FIG 0/0, 0/1), 6.3.1 (FIG 0/2), 8.1 (labels) and the header's contract: the
CRC, the walk over a FIB with its bounds, the per-FIB record, the reduction over a call's FIBs in stream order, the fields
derived from a FIG 0/1 entry, and the ETI header made from a result.  Everything is integers; the tests compare bytes."""
import struct

CRC_OK, ZERO, TRUNCATED = 1, 2, 4
REC_SUB, REC_SERVICES, REC_COMPONENTS, MAX_COMPONENTS = 9, 4, 8, 12
RECORD_BYTES, RESULT_BYTES = 288, 4320

# EN 300 401 table 6 (sub-channel size by bit rate and protection level, short form): sizes for levels 5, 4, 3, 2, 1; None = no
# such combination.  The table index counts the combinations that exist, in this order.
UEP_SIZES = [(32, (16, 21, 24, 29, 35)), (48, (24, 29, 35, 42, 52)), (56, (29, 35, 42, 52, None)), (64, (32, 42, 48, 58, 70)),
             (80, (40, 52, 58, 70, 84)), (96, (48, 58, 70, 84, 104)), (112, (58, 70, 84, 104, None)),
             (128, (64, 84, 96, 116, 140)), (160, (80, 104, 116, 140, 168)), (192, (96, 116, 140, 168, 208)),
             (224, (116, 140, 168, 208, 232)), (256, (128, 168, 192, 232, 280)), (320, (160, 208, None, 280, None)),
             (384, (192, None, 280, None, 416))]
SHORT_TABLE = [(br, 5 - i, size) for br, sizes in UEP_SIZES for i, size in enumerate(sizes) if size is not None]   # (bitrate, level, CU)
assert len(SHORT_TABLE) == 64
EEP_A, EEP_B = (12, 8, 6, 4), (27, 21, 18, 15)


def crc16(data):
    """CRC-16, x^16 + x^12 + x^5 + 1, all ones at the start, complemented at the end, bit by bit"""
    crc = 0xFFFF
    for byte in data:
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021 if crc & 0x8000 else crc << 1) & 0xFFFF
    return crc ^ 0xFFFF


assert crc16(b"123456789") == 0xD64E and crc16(bytes(30)) == 0xD5BA


def empty_record():
    return dict(flags=0, eid_first=0, eid=0, eid_seen=0, eid_changes=0, change=0, alarm=0, cif_hi=0, cif_lo=0, services_dropped=0,
                components_dropped=0, labels_dropped=0, figs_truncated=0, fig0_skipped=0, figs_type=[0] * 8, fig0_ext=[0] * 32,
                sub=[], svc=[], comp=[], label=None)


def read_fib(b):
    """32 bytes -> the record as a dictionary"""
    b = bytes(b)
    assert len(b) == 32
    r = empty_record()
    if not any(b):
        r["flags"] = ZERO
    if crc16(b[:30]) != (b[30] << 8 | b[31]):
        return r
    r["flags"] = CRC_OK
    p = 0
    while p < 30 and b[p] != 0xFF:
        typ, ln = b[p] >> 5, b[p] & 31
        if p + 1 + ln > 30:
            r["figs_truncated"] = 1
            r["flags"] |= TRUNCATED
            break
        f = b[p + 1:p + 1 + ln]                       # the FIG's field: nothing below looks outside it
        p += 1 + ln
        r["figs_type"][typ] += 1
        if not f:
            continue
        if typ == 0:
            ext = f[0] & 31
            r["fig0_ext"][ext] += 1
            if ext > 2:
                continue
            if f[0] & 0xE0:
                r["fig0_skipped"] += 1
                continue
            d = f[1:]
            if ext == 0:
                if len(d) < 4:
                    continue
                eid = d[0] << 8 | d[1]
                if not r["eid_seen"]:
                    r["eid_first"] = eid
                elif r["eid"] != eid:
                    r["eid_changes"] += 1
                r["eid"] = eid
                r["eid_seen"] += 1
                r["change"], r["alarm"], r["cif_hi"], r["cif_lo"] = d[2] >> 6, (d[2] >> 5) & 1, d[2] & 31, d[3]
            elif ext == 1:
                while len(d) >= 3:
                    long_form = d[2] >> 7
                    n = 4 if long_form else 3
                    if len(d) < n:
                        break
                    e = d[:n] + bytes(4 - n)
                    d = d[n:]
                    ent = dict(raw=int.from_bytes(e, "big"), subchid=e[0] >> 2, sad=(e[0] & 3) << 8 | e[1], form=long_form, size=0)
                    if long_form:
                        ent.update(sw_option=(e[2] >> 4) & 7, index_level=(e[2] >> 2) & 3, size=(e[2] & 3) << 8 | e[3])
                    else:
                        ent.update(sw_option=(e[2] >> 6) & 1, index_level=e[2] & 63)
                    r["sub"].append(ent)
            else:
                while len(d) >= 3:
                    nc = d[2] & 15
                    if len(d) < 3 + 2 * nc:
                        break
                    if len(r["svc"]) >= REC_SERVICES or len(r["comp"]) + nc > REC_COMPONENTS:
                        r["services_dropped"] += 1
                        r["components_dropped"] += nc
                    else:
                        for k in range(nc):
                            c0, c1 = d[3 + 2 * k], d[4 + 2 * k]
                            tmid = c0 >> 6
                            r["comp"].append(dict(tmid=tmid, type=0 if tmid == 3 else c0 & 63,
                                                  id=((c0 & 63) << 6 | c1 >> 2) if tmid == 3 else c1 >> 2,
                                                  primary=(c1 >> 1) & 1, ca=c1 & 1, service=len(r["svc"])))
                        r["svc"].append(dict(sid=d[0] << 8 | d[1], info=d[2], first_comp=len(r["comp"]) - nc))
                    d = d[3 + 2 * nc:]
        elif typ == 1:
            ext = f[0] & 7
            if f[0] & 8 or ext > 1 or len(f) != 21:
                continue
            if r["label"] is not None:
                r["labels_dropped"] += 1
                continue
            r["label"] = dict(kind=1 + ext, charset=f[0] >> 4, id=f[1] << 8 | f[2], text=f[3:19], flag=f[19] << 8 | f[20])
    assert len(r["sub"]) <= REC_SUB
    return r


def pack_record(r):
    """the 288 bytes of dabgpu_fic_record"""
    out = struct.pack("<IHH", r["flags"], r["eid_first"], r["eid"])
    out += bytes([r["eid_seen"], r["eid_changes"], r["change"], r["alarm"], r["cif_hi"], r["cif_lo"], len(r["sub"]), len(r["svc"]),
                  len(r["comp"]), r["services_dropped"], r["components_dropped"], r["labels_dropped"], r["figs_truncated"],
                  r["fig0_skipped"], 0, 0])
    out += bytes(r["figs_type"]) + bytes(r["fig0_ext"])
    for e in r["sub"]:
        out += struct.pack("<IHHBBBB", e["raw"], e["sad"], e["size"], e["subchid"], e["form"], e["sw_option"], e["index_level"])
    out += bytes(12 * (REC_SUB - len(r["sub"])))
    for s in r["svc"]:
        out += struct.pack("<HBB", s["sid"], s["info"], s["first_comp"])
    out += bytes(4 * (REC_SERVICES - len(r["svc"])))
    for c in r["comp"]:
        out += struct.pack("<HBBBBBB", c["id"], c["tmid"], c["type"], c["primary"], c["ca"], c["service"], 0)
    out += bytes(8 * (REC_COMPONENTS - len(r["comp"])))
    lab = r["label"]
    out += struct.pack("<BBHH16sH", lab["kind"], lab["charset"], lab["id"], lab["flag"], lab["text"], 0) if lab else bytes(24)
    out += bytes(12)
    assert len(out) == RECORD_BYTES
    return out


def derive(raw):
    """the fields of dabgpu_fic_subch that follow from a FIG 0/1 entry's raw word"""
    b = raw.to_bytes(4, "big")
    s = dict(subchid=b[0] >> 2, sad=(b[0] & 3) << 8 | b[1], size_cu=0, form=b[2] >> 7, index_option=0, level=0, bitrate=0, tpl=0,
             stl=0, supported=0, raw=raw, table_switch=0)
    if not s["form"]:
        s["table_switch"], s["index_option"] = (b[2] >> 6) & 1, b[2] & 63
        if not s["table_switch"]:
            s["bitrate"], s["level"], s["size_cu"] = SHORT_TABLE[s["index_option"]]
            s["tpl"], s["supported"] = s["level"] - 1, 1
    else:
        s["index_option"], s["level"], s["size_cu"] = (b[2] >> 4) & 7, ((b[2] >> 2) & 3) + 1, (b[2] & 3) << 8 | b[3]
        if s["index_option"] <= 1:
            f = (EEP_B if s["index_option"] else EEP_A)[s["level"] - 1]
            if s["size_cu"] and s["size_cu"] % f == 0:
                s["bitrate"] = s["size_cu"] // f * (32 if s["index_option"] else 8)
                s["tpl"], s["supported"] = 0x20 | s["index_option"] << 2 | (s["level"] - 1), 1
    s["stl"] = 3 * s["bitrate"] // 8
    return s


class Run:
    """what one pass over the sightings of a key gives"""
    def __init__(self):
        self.last = self.seen = self.changes = self.first_fib = self.last_fib = 0

    def see(self, word, fib):
        if self.seen and word != self.last:
            self.changes += 1
        if not self.seen:
            self.first_fib = fib
        self.last, self.last_fib = word, fib
        self.seen += 1


def scan(fibs):
    """FIBs in stream order (an iterable of 32 bytes each) -> (records, result): the dictionaries of read_fib and the
    dictionary of dabgpu_fic_result (sub: the SubChIds seen, ascending)"""
    recs = [read_fib(f) for f in fibs]
    res = dict(fibs=len(recs), fibs_ok=0, fibs_bad=0, fibs_zero=0, figs_truncated=0, fig0_skipped=0, services_dropped=0,
               components_dropped=0, labels_dropped=0, figs_type=[0] * 8, fig0_ext=[0] * 32)
    eid, subs = Run(), [Run() for _ in range(64)]
    for i, r in enumerate(recs):
        ok = bool(r["flags"] & CRC_OK)
        res["fibs_ok"] += ok
        res["fibs_zero"] += bool(r["flags"] & ZERO)
        res["fibs_bad"] += not ok and not r["flags"] & ZERO
        for k in ("figs_truncated", "fig0_skipped", "services_dropped", "components_dropped", "labels_dropped"):
            res[k] += r[k]
        for name in ("figs_type", "fig0_ext"):
            res[name] = [a + b for a, b in zip(res[name], r[name])]
        if r["eid_seen"]:
            # (within the FIB: first, changes and last are the record's)
            if eid.seen and r["eid_first"] != eid.last:
                eid.changes += 1
            if not eid.seen:
                eid.first_fib = i
            eid.changes += r["eid_changes"]
            eid.seen += r["eid_seen"]
            eid.last, eid.last_fib = r["eid"], i
        for e in r["sub"]:
            subs[e["subchid"]].see(e["raw"], i)
    res.update(eid=eid.last, eid_seen=eid.seen, eid_changes=eid.changes, eid_first_fib=eid.first_fib, eid_last_fib=eid.last_fib)
    res["sub"] = []
    for run in subs:
        if run.seen:
            s = derive(run.last)
            s.update(seen=run.seen, changes=run.changes, first_fib=run.first_fib, last_fib=run.last_fib)
            res["sub"].append(s)
    res["n_subch"] = len(res["sub"])
    return recs, res


SUBCH_FIELDS = ("subchid", "sad", "size_cu", "form", "index_option", "level", "bitrate", "tpl", "stl", "supported", "seen",
                "changes", "first_fib", "last_fib", "raw", "table_switch")


def pack_result(res):
    """the 4320 bytes of dabgpu_fic_result"""
    head = [res[k] for k in ("fibs", "fibs_ok", "fibs_bad", "fibs_zero", "figs_truncated", "fig0_skipped", "services_dropped",
                             "components_dropped", "labels_dropped", "eid", "eid_seen", "eid_changes", "eid_first_fib",
                             "eid_last_fib", "n_subch")] + [0]
    out = struct.pack("<16I", *head) + struct.pack("<8I", *res["figs_type"]) + struct.pack("<32I", *res["fig0_ext"])
    for s in res["sub"]:
        out += struct.pack("<16I", *[s[k] for k in SUBCH_FIELDS])
    out += bytes(64 * (64 - len(res["sub"])))
    assert len(out) == RESULT_BYTES
    return out


def services(recs):
    """(ensemble label or None, services in order of first appearance) as Modulator.fic_services() reports them"""
    ens, found = None, []

    def service(sid):
        for s in found:
            if s["sid"] == sid:
                return s
        found.append(dict(sid=sid, sightings=0, components_dropped=0, label=None, components=[]))
        return found[-1]

    for r in recs:
        if not r["flags"] & CRC_OK:
            continue
        for sv in r["svc"]:
            s = service(sv["sid"])
            s["sightings"] += 1
            for c in r["comp"][sv["first_comp"]:sv["first_comp"] + (sv["info"] & 15)]:
                new = {k: c[k] for k in ("id", "tmid", "type", "primary", "ca")}
                at = [x for x in s["components"] if (x["tmid"], x["id"]) == (c["tmid"], c["id"])]
                if at:
                    at[0].update(new)
                elif len(s["components"]) >= MAX_COMPONENTS:
                    s["components_dropped"] += 1
                else:
                    s["components"].append(new)
        lab = r["label"]
        if lab and lab["kind"] == 1:
            ens = dict(lab)
        if lab and lab["kind"] == 2:
            service(lab["id"])["label"] = dict(lab)
    return ens, found


def fibs_of(images, fic_offset, fic_bytes):
    """(n, 6144) uint8 -> the FIBs in stream order"""
    return [bytes(bytearray(im[fic_offset + 32 * i:fic_offset + 32 * i + 32])) for im in images for i in range(fic_bytes // 32)]


MID = {1: 1, 2: 2, 3: 3, 4: 0}


def header_refusal(res):
    """the start of the message dabgpu_fic_make_header refuses this result with, before it looks at the layout; None: it goes on"""
    if res["n_subch"] == 0:
        return "fic: no sub-channel organisation seen"
    if res["n_subch"] > 64:
        return "fic: more than 64 sub-channels"
    for s in res["sub"]:
        if s["changes"]:
            return "fic: sub-channel %d was redefined inside the capture" % s["subchid"]
        if not s["supported"]:
            return "fic: sub-channel %d is not supported" % s["subchid"]
    return None


def make_header(res, mode):
    """the 6144 bytes dabgpu_fic_make_header writes for a result it does not refuse"""
    fic = 128 if mode == 3 else 96
    subs = res["sub"]
    mst = sum(8 * s["stl"] for s in subs)
    fl = (4 * len(subs) + 4 + fic + mst) // 4
    f = bytearray([0x55] * 6144)
    f[0:8] = bytes([0xFF, 0x07, 0x3A, 0xB6, 0, 0x80 | len(subs), MID[mode] << 3 | (fl >> 8) & 7, fl & 0xFF])
    p = 8
    for s in subs:
        f[p:p + 4] = bytes([s["subchid"] << 2 | s["sad"] >> 8, s["sad"] & 0xFF, s["tpl"] << 2 | s["stl"] >> 8, s["stl"] & 0xFF])
        p += 4
    body = 4 + fic + mst
    if p + body + 8 <= 6144:
        f[p:p + body] = bytes(body)
        p += body
        f[p:p + 8] = bytes([0, 0, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF])
    return bytes(f)
