"""Files without their DHT tables, shared by tests/test_jpeg_std_tables.py, scripts/make_jpeg_std_corpus.py and the GPU tests of the
std_tables option: what a UVC camera in MJPG mode or an MJPG AVI frame looks like.  Pillow writes a file with the standard (Annex K.3)
tables; `strip` walks its segments up to the SOS and removes the tables named, one by one, a DHT segment that ends up empty altogether."""
from jpeg_dec_cases import pillow_file

# what is removed, as (class, slot): class 0 DC, 1 AC; slot 0 luminance, 1 chrominance
VARIANTS = {
    'all': {(0, 0), (0, 1), (1, 0), (1, 1)},
    'chroma': {(0, 1), (1, 1)},
    'luma': {(0, 0), (1, 0)},
    'dc0': {(0, 0)},
    'ac0_dc1': {(1, 0), (0, 1)},
}
SAMPLINGS = ['4:2:0', '4:2:2', '4:4:4', 'L']
SIZES = [(16, 16), (17, 33), (40, 56), (3, 5)]          # (height, width)


def strip(data, remove):
    """`data` without the DHT tables in `remove`; every other byte as it was."""
    d = bytes(data)
    assert d[:2] == b'\xff\xd8'
    out, i = bytearray(d[:2]), 2
    while True:
        assert d[i] == 0xFF, 'no marker at %d' % i
        m = d[i + 1]
        L = (d[i + 2] << 8) | d[i + 3]
        if m == 0xC4:
            p, e, kept = i + 4, i + 2 + L, bytearray()
            while p < e:
                n = 17 + sum(d[p + 1:p + 17])
                if (d[p] >> 4, d[p] & 15) not in remove:
                    kept += d[p:p + n]
                p += n
            assert p == e
            if kept:
                out += bytes([0xFF, 0xC4, (len(kept) + 2) >> 8, (len(kept) + 2) & 255]) + kept
        else:
            out += d[i:i + 2 + L]
        i += 2 + L
        if m == 0xDA:
            return bytes(out + d[i:])


def standard_file(H, W, sampling, kind='noise', restart='none', progressive=False, seed=0):
    """Quality 75, standard tables (optimize off), as the issue's check on Pillow used."""
    return pillow_file(H, W, kind, 75, sampling, restart, False, seed, progressive)


def referenced(sampling, remove):
    """The tables of `remove` a file of this sampling reads at all (a greyscale file reads slot 0 only)."""
    return {t for t in remove if sampling != 'L' or t[1] == 0}
