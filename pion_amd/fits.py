"""Reader of the FITS files the C++ host loop writes (pion_host_sim_write_fits, pion_amd/host/fits_io.h), numpy only.

    params, images = fits.read(path)

params: every parameter of the primary header under the name the PIONRAW2 header gives it -- integers as int, reals
as float (bit for bit what the run held: they are printed with %.17G), strings as str; the element-numbered cards of
an array (NGrid0, NGrid1, ...) are joined into a list under the array's name (NGrid).  images: EXTNAME -> ndarray of
float64 in native byte order, shaped [NAXIS3][NAXIS2][NAXIS1] (x fastest).  Bx, By, Bz and divB carry the factor
sqrt(4 pi) the reference writes; psi and Ptot do not.

It reads what that writer produces (double-precision IMAGE extensions, HIERARCH cards, CONTINUE'd strings), not FITS
in general."""
import re

import numpy as np

BLOCK, CARD = 2880, 80
ARRAY_KEYS = ("NGrid", "Xmin", "Xmax", "Ref_Vector")


def _parse_value(text):
    """value field of a card: (python value, the string continues on the next card)"""
    text = text.strip()
    if text.startswith("'"):
        # up to the closing quote; a doubled quote is a quote
        out, i = [], 1
        while i < len(text):
            if text[i] == "'":
                if i + 1 < len(text) and text[i + 1] == "'":
                    out.append("'")
                    i += 2
                    continue
                break
            out.append(text[i])
            i += 1
        s = "".join(out)
        if s.endswith("&"):
            return s[:-1], True
        return s.rstrip(" "), False
    text = text.split("/")[0].strip()
    if text in ("T", "F"):
        return text == "T", False
    if re.fullmatch(r"[+-]?\d+", text):
        return int(text), False
    return float(text), False


def _read_header(raw, pos):
    """cards from byte pos up to END: ([(keyword, value)], first byte after the header's last block)"""
    cards, last = [], None
    while True:
        block = raw[pos:pos + BLOCK]
        if len(block) < BLOCK:
            raise ValueError("FITS header without END")
        pos += BLOCK
        for i in range(0, BLOCK, CARD):
            c = block[i:i + CARD].decode("ascii")
            if c.startswith("END") and not c[3:].strip():
                return cards, pos
            if c.startswith("CONTINUE"):
                if last is None or not last[2]:
                    raise ValueError("CONTINUE card without a string to continue")
                v, more = _parse_value(c[8:])
                last[1] += v
                last[2] = more
                continue
            if c.startswith("HIERARCH "):
                key, _, val = c[9:].partition("=")
            elif c[8:10] == "= ":
                key, val = c[:8], c[10:]
            else:
                continue   # comment or blank card
            v, more = _parse_value(val)
            last = [key.strip(), v, more]
            cards.append(last)


def read(path):
    """(params: dict, images: dict name -> ndarray) of a file written by pion_host_sim_write_fits"""
    raw = open(path, "rb").read()
    cards, pos = _read_header(raw, 0)
    kv = [(k, v) for k, v, _ in cards]
    if kv[:1] != [("SIMPLE", True)]:
        raise ValueError("%s is not a FITS file" % path)
    params = {}
    for k, v in kv[4:]:
        m = re.fullmatch(r"(%s)(\d+)" % "|".join(ARRAY_KEYS), k)
        if m:
            params.setdefault(m.group(1), []).append(v)
        else:
            params[k] = v
    images = {}
    while pos < len(raw):
        cards, pos = _read_header(raw, pos)
        h = {k: v for k, v, _ in cards}
        if h.get("XTENSION") != "IMAGE" or h.get("BITPIX") != -64:
            raise ValueError("%s: only double-precision IMAGE extensions are read" % path)
        shape = [h["NAXIS%d" % (a + 1)] for a in range(h["NAXIS"])][::-1]
        n = int(np.prod(shape)) * 8
        images[h["EXTNAME"]] = np.frombuffer(raw, dtype=">f8", count=n // 8, offset=pos).reshape(shape).astype("=f8")
        pos += (n + BLOCK - 1) // BLOCK * BLOCK
    return params, images
