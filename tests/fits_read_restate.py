"""What the FITS restart tests share: a numpy restatement of what the reference's FITS reader stores in the state for a
file, and the few helpers that take a FITS file apart and put it together again.  Not a test module.  It shares no
code with pion_amd/fits.py or the C++ reader, and needs nothing outside this repository.

The restatement, rule by rule (reference lines; none of its text is copied):
  which images  dataIO/dataio_fits.cpp:433-548: the nvar primitive images GasDens GasPres GasVX GasVY GasVZ [Bx By Bz
                [psi]] TR0.., each looked up by its name; Eint / Temp, divB, Ptot are never read (:901-903)
  missing image the variable is zero everywhere (:505-512)
  an element    the big-endian double of the file as a native double; for Bx, By, Bz times 1.0/sqrt(4.0*M_PI), a
                multiplication (:911-916); psi is not scaled
  rejected      the file element (before the scaling) is not finite, or constants::equalD(x, -1.e99) holds for it
                (:908-921, constants.cpp:48-70)
numpy evaluates each of these element by element in IEEE double, in the order written."""
import numpy as np

import fits_restate as fr
from pion_amd import abi

BLOCK, CARD = 2880, 80
BINV = 1.0 / np.sqrt(4.0 * np.pi)
NULVAL = -1.0e99


def prim_names(cfg):
    return fr.image_names(cfg)[:cfg.nvar]


def is_b(cfg, v):
    return cfg.eqntype in (abi.EQMHD, abi.EQGLM) and abi.BX <= v <= abi.BZ


def rejected(x):
    """elementwise: not finite, or equalD(x, -1e99)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = np.abs(x)
        eq = (x == NULVAL) | (a + abs(NULVAL) < 1.0e-100) | (np.abs(x - NULVAL) / (a + abs(NULVAL) + 1.0e-100) < 1.0e-12)
    return ~np.isfinite(x) | eq


def stored(cfg, v, x):
    """what the state holds for file elements x (native doubles) of variable v"""
    x = np.asarray(x, dtype=np.float64)
    return x * BINV if is_b(cfg, v) else x.copy()


def from_big_endian(cfg, buf):
    """a buffer [nvar][...] of file elements (dtype '>f8') -> (state values [nvar][...], number of rejected elements)"""
    buf = np.asarray(buf)
    assert buf.dtype == np.dtype(">f8") and buf.shape[0] == cfg.nvar
    x = buf.astype("=f8")
    return np.stack([stored(cfg, v, x[v]) for v in range(cfg.nvar)]), int(rejected(x).sum())


# ---- a FITS file as a list of HDUs ------------------------------------------------------------------------------

def split_hdus(raw):
    """[(header bytes, data bytes with their padding)] of a file, every data unit sized from its own header"""
    pos, out = 0, []
    while pos < len(raw):
        h0, kv = pos, {}
        while True:
            block = raw[pos:pos + BLOCK]
            assert len(block) == BLOCK, "header without END"
            pos += BLOCK
            cards = [block[i:i + CARD].decode("ascii") for i in range(0, BLOCK, CARD)]
            for c in cards:
                if c[8:10] == "= " and not c.startswith("HIERARCH"):
                    kv.setdefault(c[:8].strip(), c[10:].split("/")[0].strip())
            if any(c.rstrip() == "END" for c in cards):
                break
        n = 0
        if int(kv.get("NAXIS", 0)) > 0:
            n = 1
            for a in range(int(kv["NAXIS"])):
                n *= int(kv["NAXIS%d" % (a + 1)])
        n = abs(int(kv["BITPIX"])) // 8 * int(kv.get("GCOUNT", 1)) * (int(kv.get("PCOUNT", 0)) + n)
        padded = (n + BLOCK - 1) // BLOCK * BLOCK
        out.append((raw[h0:pos], raw[pos:pos + padded]))
        pos += padded
    return out


def extname(header):
    for i in range(0, len(header), CARD):
        c = header[i:i + CARD].decode("ascii")
        if c.startswith("EXTNAME ="):
            return c[10:].strip().strip("'").strip()
    return None


def join_hdus(hdus):
    return b"".join(h + d for h, d in hdus)


def replace_card(header, start, new):
    """the header with the one card that begins with `start` replaced by the card `new`"""
    cards = [header[i:i + CARD] for i in range(0, len(header), CARD)]
    hit = [i for i, c in enumerate(cards) if c.startswith(start.encode())]
    assert len(hit) == 1, (start, len(hit))
    cards[hit[0]] = new.encode().ljust(CARD)
    assert len(cards[hit[0]]) == CARD
    return b"".join(cards)


def fixed_card(key, value):
    return "%-8s= %20s" % (key, value)


def plant(data, index, value):
    """the data unit with element `index` set to the big-endian double `value`"""
    return data[:8 * index] + np.array([value], dtype=">f8").tobytes() + data[8 * index + 8:]


def foreign_hdu():
    """an extension no restart needs: a binary table of 7 x 3 bytes with a 5-byte heap, filled with non-zero bytes"""
    cards = ["XTENSION= 'BINTABLE'", fixed_card("BITPIX", 8), fixed_card("NAXIS", 2), fixed_card("NAXIS1", 7),
             fixed_card("NAXIS2", 3), fixed_card("PCOUNT", 5), fixed_card("GCOUNT", 1), fixed_card("TFIELDS", 1),
             "TFORM1  = '7A      '", "EXTNAME = 'GasDens_notes'", "COMMENT an HDU of somebody else's", "END"]
    h = "".join(c.ljust(CARD) for c in cards).encode().ljust(BLOCK)
    return h, (b"\x7f" * 26).ljust(BLOCK, b"\0")


# ---- the primary header's parameters, as far as the tests need them (numbers only) ---------------------------------

def params(path):
    """{name: int or float} of the HIERARCH cards of the primary header that hold a number"""
    raw = open(path, "rb").read()
    out = {}
    for i in range(0, len(split_hdus(raw)[0][0]), CARD):
        c = raw[i:i + CARD].decode("ascii")
        if not c.startswith("HIERARCH "):
            continue
        k, _, v = c[9:].partition("=")
        v = v.strip()
        if v.startswith("'"):
            continue
        out[k.strip()] = int(v) if v.lstrip("+-").isdigit() else float(v)
    return out


# ---- the state a restart from these files holds --------------------------------------------------------------------

def restate_files(cfg, paths):
    """(on-grid state [nvar][nz][ny][nx] of the global problem `cfg`, rejected elements, missing image names, params
    of the first file): every plane from the first file that holds it"""
    nplanes = 1 if cfg.ndim == 1 else cfg.ng[cfg.ndim - 1]
    ax = {3: 1, 2: 2, 1: None}[cfg.ndim]   # axis of the planes in [nvar][nz][ny][nx]
    shape = (cfg.nvar, cfg.ng[2], cfg.ng[1], cfg.ng[0])
    out, have = np.zeros(shape), np.zeros(nplanes, dtype=bool)
    nbad, missing = 0, []
    for p in paths:
        par = params(p)
        lo, n = par.get("pion_slab_lo", 0), par.get("pion_slab_n", nplanes)
        images = fr.images_of(p)
        take = [k for k in range(lo, lo + n) if not have[k]]
        for v, name in enumerate(prim_names(cfg)):
            if name not in images:
                missing.append(name)
                continue   # zeros
            img = images[name]
            nbad += int(rejected(img).sum()) if take else 0
            val = stored(cfg, v, img)
            for k in take:
                if ax is None:
                    out[v, 0, 0, :] = val
                elif ax == 1:
                    out[v, k] = val[k - lo]
                else:
                    out[v, 0, k] = val[k - lo]
        have[take] = True
    assert have.all()
    return out, nbad, missing, params(paths[0])


def embed(cfg, og):
    """the all-cell array [nvar][nz_all][ny_all][nx_all] with zero ghost cells around the on-grid state"""
    from pion_amd import problems
    A = np.zeros(problems.alloc(cfg).shape)
    nb = cfg.nbc
    sl = tuple(slice(nb, -nb) if a < cfg.ndim else slice(None) for a in (2, 1, 0))
    A[(slice(None),) + sl] = og
    return A
