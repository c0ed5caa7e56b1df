"""Inputs shared by tests/test_fic_cpu.py and tests/test_fic_gpu.py: a FIG / FIB builder (EN 300 401 5.2, 6.2.1, 6.3.1, 8.1) and
with_fic, which writes into a synth_eti stream a FIC that says what the stream's own STC words say."""
import numpy as np

from tests import fic_model as FM


def fig(typ, field=b""):
    field = bytes(field)
    assert len(field) <= 31
    return bytes([typ << 5 | len(field)]) + field


def fig0(ext, field=b"", cn=0, oe=0, pd=0):
    return fig(0, bytes([cn << 7 | oe << 6 | pd << 5 | ext]) + bytes(field))


def fig0_0(eid, change=0, alarm=0, cif_hi=0, cif_lo=0, **flags):
    return fig0(0, bytes([eid >> 8, eid & 0xFF, change << 6 | alarm << 5 | cif_hi, cif_lo]), **flags)


def sub_short(subchid, sad, index, switch=0):
    return bytes([subchid << 2 | sad >> 8, sad & 0xFF, switch << 6 | index])


def sub_long(subchid, sad, option, level, size):
    """level: the 2-bit field, 0 ... 3 for protection levels 1 ... 4"""
    return bytes([subchid << 2 | sad >> 8, sad & 0xFF, 0x80 | option << 4 | level << 2 | size >> 8, size & 0xFF])


def fig0_1(entries, **flags):
    return fig0(1, b"".join(entries), **flags)


def component(tmid, typ, ident, primary=1, ca=0):
    """TMId 0 ... 2: (ASCTy / DSCTy, SubChId); TMId 3: ident is the 12-bit SCId"""
    if tmid == 3:
        return bytes([0xC0 | ident >> 6, (ident & 63) << 2 | primary << 1 | ca])
    return bytes([tmid << 6 | typ, ident << 2 | primary << 1 | ca])


def service(sid, components, local=0, caid=0):
    return bytes([sid >> 8, sid & 0xFF, local << 7 | caid << 4 | len(components)]) + b"".join(components)


def fig0_2(services, **flags):
    return fig0(2, b"".join(services), **flags)


def fig1(ext, ident, text, flag=0xFF00, charset=0, oe=0):
    text = bytes(text).ljust(16)[:16]
    return fig(1, bytes([charset << 4 | oe << 3 | ext, ident >> 8, ident & 0xFF]) + text + bytes([flag >> 8, flag & 0xFF]))


def fib(figs=(), crc=True):
    """FIGs, the end marker and zero padding where there is room, the CRC (crc=False: one wrong)"""
    body = b"".join(figs)
    assert len(body) <= 30
    if len(body) < 30:
        body += b"\xff" + bytes(29 - len(body))
    c = FM.crc16(body) ^ (0 if crc else 0x0100)
    return body + bytes([c >> 8, c & 0xFF])


def flip(f, bit):
    """a FIB with one bit flipped (bit 0 = the highest bit of byte 0)"""
    f = bytearray(f)
    f[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(f)


def entry_of(subchid, sad, stl, tpl):
    """the FIG 0/1 entry that says what an STC word (SAD, STL, TPL) says: UEP in the short form, EEP in the long form"""
    bitrate = stl * 8 // 3
    if tpl & 0x20:
        option, level = (tpl >> 2) & 7, tpl & 3
        factor, unit = ((FM.EEP_A, 8), (FM.EEP_B, 32))[option]
        return sub_long(subchid, sad, option, level, bitrate // unit * factor[level])
    index = [i for i, (br, lvl, _) in enumerate(FM.SHORT_TABLE) if (br, lvl) == (bitrate, tpl + 1)]
    return sub_short(subchid, sad, index[0])


def images_of(fibs, fic_offset=12, fibs_per_image=3, fill=0xA5):
    """FIBs in stream order -> (n, 6144) images with the FIC at fic_offset and `fill` everywhere else"""
    assert len(fibs) % fibs_per_image == 0
    out = np.full((len(fibs) // fibs_per_image, 6144), fill, np.uint8)
    flat = np.frombuffer(b"".join(fibs), np.uint8).reshape(-1, 32 * fibs_per_image)
    out[:, fic_offset:fic_offset + 32 * fibs_per_image] = flat
    return out


def stc_of(frame):
    """the (SAD, STL, TPL) of an ETI frame's STC words, in STC order"""
    nst = int(frame[5]) & 0x7F
    out = []
    for i in range(nst):
        s = [int(x) for x in frame[8 + 4 * i:12 + 4 * i]]
        out.append(((s[0] & 3) << 8 | s[1], (s[2] & 3) << 8 | s[3], s[2] >> 2))
    return out


def with_fic(eti, mode, subchids=None, eid=0x4FFF):
    """A copy of a synth_eti stream with a real FIC: every ETI frame carries FIG 0/0 and the FIG 0/1 entries of the stream's own
    STC words (SubChId = the STC index, or subchids[i]), as many to a FIB as fit; the FIBs left over carry a FIG 0/2 with one audio
    service for each of the first four sub-channels and the labels in turn, or nothing but the end marker."""
    eti = np.array(eti, np.uint8, copy=True)
    stc = stc_of(eti[0])
    ids = list(range(len(stc))) if subchids is None else list(subchids)
    entries = [entry_of(ids[i], *stc[i]) for i in range(len(stc))]
    fibs_per = 4 if mode == 3 else 3
    fic_offset = 12 + 4 * len(stc)
    groups, room = [[]], 30 - 6 - 2                 # (FIB 0: FIG 0/0 takes six bytes, a FIG 0/1's two headers two)
    for e in entries:
        if len(e) > room:
            groups.append([])
            room = 30 - 2
        groups[-1].append(e)
        room -= len(e)
    assert len(groups) <= fibs_per
    for n in range(eti.shape[0]):
        fibs = [fib([fig0_0(eid, cif_hi=(n // 250) % 20, cif_lo=n % 250)] * (g == 0) + [fig0_1(grp)]) for g, grp in enumerate(groups)]
        if len(fibs) < fibs_per and ids:
            svc = [service(0x1000 + i, [component(0, 63, i)]) for i in ids[:4]]
            fibs.append(fib([fig0_2(svc)]))
        if len(fibs) < fibs_per:
            k = n % (len(ids) + 1)
            fibs.append(fib([fig1(0, eid, b"Ensemble") if k == 0 else fig1(1, 0x1000 + ids[k - 1], b"Service %d" % ids[k - 1])]))
        while len(fibs) < fibs_per:
            fibs.append(fib())
        eti[n, fic_offset:fic_offset + 32 * fibs_per] = np.frombuffer(b"".join(fibs), np.uint8)
    return eti
