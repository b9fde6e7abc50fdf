"""What tests/test_jpeg_scans.py, tests/test_jpeg_default_tables.py and tools/jpeg_scans_rate.py share: multi-scan sequential JPEG files
(melf_ctx_set_jpeg_multiscan) and files without their Huffman tables (melf_ctx_set_jpeg_default_tables), built from tests/jpeg_writer.py
without a new entropy coder.  A non-interleaved scan of a component is, bit for bit, the entropy-coded segment of a greyscale file of
the component's size whose blocks are the component's real blocks: `write_jpeg` with the greyscale sampling writes exactly that, so a
multi-scan file is SOI, DQT, the three-component SOF, then per scan [DHT] [DRI] SOS and the segment cut out of such a file, then EOI.
The interleaved twin is `write_jpeg` on the same grids; the reference frame is Pillow's (libjpeg-turbo's) decode, never the GPU's."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # the tool imports this module from tools/, without the package
import jpeg_sampling_cases as sc  # noqa: E402
import jpeg_writer as jw  # noqa: E402

(TAKE_ORIENT, TAKE_PROG, TAKE_SAMP, TAKE_TABLES, TAKE_MULTI) = (1, 2, 4, 16, 32)
OLD_REASON = 'more than one scan (non-interleaved components)'
OLD_TABLE_REASON = 'missing Huffman table'
SIZES = [(8, 8), (16, 16), (37, 51), (33, 130), (70, 19)]      # these cut the MCU in both directions: real grid narrower than the padded one
ORDERS = [(0, 1, 2), (2, 0, 1), (1, 2, 0)]                     # Y Cb Cr, Cr Y Cb, Cb Cr Y
RESTARTS = ['none', 'one', 'seven', 'row', 'mixed']
TABLES = ['ids01', 'ids23', 'redefined']
ALL_TABLES = (('dc', 0), ('ac', 0), ('dc', 1), ('ac', 1))


def samplings_of(size):
    return ['444', '422', '420'] + (['411', '440'] if size in ((33, 130), (70, 19)) else [])


def component_size(size, sampling, c):
    (H, W) = size
    (_nc, hs, vs) = jw.SAMPLING[sampling]
    return (H, W) if c == 0 else (-(-H // vs), -(-W // hs))


def real_grid(size, sampling, c):
    (h, w) = component_size(size, sampling, c)
    return (-(-h // 8), -(-w // 8))


def segments(data):
    """[(marker, offset of its FF, offset behind its parameters)] of the header segments up to and including the first SOS."""
    out = []
    i = 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        L = (data[i + 2] << 8) | data[i + 3]
        out.append((m, i, i + 2 + L))
        i += 2 + L
        if m == 0xDA:
            return out


def entropy_segment(data):
    """The entropy-coded bytes of a single-scan writer file: behind its SOS parameters, up to its EOI."""
    assert data[-2:] == b'\xff\xd9'
    return data[segments(data)[-1][2]:-2]


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(payload)


def _dht(kind, tid, spec):
    return _seg(0xC4, bytes([(0x10 if kind == 'ac' else 0) | tid]) + bytes(spec[0][1:17]) + bytes(spec[1]))


def scan_bytes(grid, csize, qt, spec_dc, spec_ac, restart):
    """One component's real-block grid as the entropy-coded segment of a greyscale file of the component's size."""
    data = jw.write_jpeg([np.ascontiguousarray(grid)], csize, 'grey', {0: qt}, {0: spec_dc}, {0: spec_ac}, restart=restart)
    return entropy_segment(data)


def write_multiscan(coefs, size, sampling, qt=sc.QT, order=(0, 1, 2), tables=None, restarts=(0, 0, 0), sof=0xC0, hoist=True, omit=(),
                    between=(), scans=None, tail=b'', dqt_late=False):
    """A multi-scan sequential file of MCU-padded coefficient grids.
    order      the components in the order their scans are sent
    tables     per COMPONENT (td, ta, DC spec, AC spec); default: luma on the Annex K luminance tables with ids 0 / 0, chroma on the
               chrominance tables with ids 1 / 1
    restarts   per COMPONENT the restart interval of its scan, in blocks (0: none); a DRI stands in front of a scan whose interval
               differs from the one in force
    hoist      all DHT segments in front of the first SOS (needs one definition per id); else each scan's two tables in front of its SOS
    omit       tables used for coding but not written: ('dc' | 'ac', id)
    between    segments put in front of the second and third scan's own (COM, APPn)
    scans      the scripts the decoder refuses: a list of (component, ...) tuples that replaces `order`; a tuple of two components
               writes an SOS of two components over the first one's bytes
    tail       bytes between the last scan and EOI;  dqt_late: a DQT segment behind the first scan"""
    (H, W) = size
    (nc, hs, vs) = jw.SAMPLING[sampling]
    assert nc == 3
    std = jw.standard_tables()
    if tables is None:
        tables = [(0, 0, std['dc'][0], std['ac'][0])] + [(1, 1, std['dc'][1], std['ac'][1])] * 2
    out = bytearray(b'\xff\xd8')
    out += _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in sorted(qt):
        out += _seg(0xDB, jw._dqt_payload(t, qt[t][0], qt[t][1]))
    frame = bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big') + bytes([3])
    for c in range(3):
        frame += bytes([c + 1, ((hs << 4) | vs) if c == 0 else 0x11, 0 if c == 0 else 1])
    out += _seg(sof, frame)
    if hoist:
        seen = {}
        for (td, ta, sd, sa) in tables:
            for (kind, tid, spec) in (('dc', td, sd), ('ac', ta, sa)):
                assert seen.setdefault((kind, tid), spec) == spec, 'hoist needs one definition per table id'
        for ((kind, tid), spec) in sorted(seen.items()):
            if (kind, tid) not in omit:
                out += _dht(kind, tid, spec)
    in_force = 0
    for (k, item) in enumerate(scans if scans is not None else [(c,) for c in order]):
        c = item[0]
        (td, ta, sd, sa) = tables[c]
        if k:
            for s in between:
                out += s
            if dqt_late and k == 1:
                out += _seg(0xDB, jw._dqt_payload(1, qt[1][0], qt[1][1]))
        if not hoist:
            for (kind, tid, spec) in (('dc', td, sd), ('ac', ta, sa)):
                if (kind, tid) not in omit:
                    out += _dht(kind, tid, spec)
        if restarts[c] != in_force:
            out += _seg(0xDD, int(restarts[c]).to_bytes(2, 'big'))
            in_force = restarts[c]
        sos = bytes([len(item)])
        for q in item:
            sos += bytes([q + 1, (tables[q][0] << 4) | tables[q][1]])
        out += _seg(0xDA, sos + bytes([0, 63, 0]))
        (by, bx) = real_grid(size, sampling, c)
        out += scan_bytes(coefs[c][:by, :bx], component_size(size, sampling, c), qt[0 if c == 0 else 1], sd, sa, restarts[c])
    return bytes(out) + bytes(tail) + b'\xff\xd9'


def restart_plan(name, size, sampling):
    """Per component the restart interval of the plan `name`."""
    rows = [real_grid(size, sampling, c)[1] for c in range(3)]
    return {'none': (0, 0, 0), 'one': (1, 1, 1), 'seven': (7, 7, 7), 'row': tuple(rows), 'mixed': (3, 0, 5)}[name]


def table_plan(name):
    """(tables, sof, hoist) of the plan `name`.  'redefined': every scan uses ids 0 / 0, and each scan's DHT redefines them with
    another code set -- luminance, chrominance, and a length-limited set of its own -- so that a decoder which took one definition
    for all three scans would decode garbage."""
    std = jw.standard_tables()
    (ld, la, cd, ca) = (std['dc'][0], std['ac'][0], std['dc'][1], std['ac'][1])
    if name == 'ids01':
        return ([(0, 0, ld, la), (1, 1, cd, ca), (1, 1, cd, ca)], 0xC0, True)
    if name == 'ids23':
        return ([(2, 2, ld, la), (3, 3, cd, ca), (3, 3, cd, ca)], 0xC1, True)
    assert name == 'redefined'
    flat_dc = jw.tables_from_lengths({4: list(range(12))})          # a third DC code set: twelve 4-bit codes
    return ([(0, 0, ld, la), (0, 0, cd, ca), (0, 0, flat_dc, la)], 0xC0, False)


def grids_for(size, sampling, seed=3):
    rng = np.random.default_rng(seed + 1000 * size[0] + size[1])
    return sc.image_coefs(sc.natural(rng, *size), sampling)


def decode_cases(size):
    """[(name, multi-scan bytes, twin bytes)] for one size: every sampling, scan order, restart plan and table plan."""
    out = []
    for sampling in samplings_of(size):
        grids = grids_for(size, sampling)
        twin = sc.write(grids, size, sampling)
        for (a, order) in enumerate(ORDERS):
            for (b, rname) in enumerate(RESTARTS):
                for (t, tname) in enumerate(TABLES):
                    (tables, sof, hoist) = table_plan(tname)
                    between = (_seg(0xFE, b'between the scans'), _seg(0xE7, bytes(range(40)))) if (a + b + t) % 3 == 0 else ()
                    data = write_multiscan(grids, size, sampling, order=order, tables=tables, restarts=restart_plan(rname, size, sampling),
                                           sof=sof, hoist=hoist, between=between)
                    out.append(('%dx%d-%s-%s-%s-%s' % (size[0], size[1], sampling, ''.join('YBR'[c] for c in order), rname, tname), data, twin))
    return out


def refusal_cases(size=(37, 51), sampling='420'):
    """{name: bytes}: the scripts that stay unsupported with the switch on."""
    grids = grids_for(size, sampling)
    com = _seg(0xFE, b'behind the third scan')
    return {
        'two components in a scan': write_multiscan(grids, size, sampling, scans=[(0,), (1, 2)]),
        'component sent twice': write_multiscan(grids, size, sampling, scans=[(0,), (1,), (1,)]),
        'ends before the third scan': write_multiscan(grids, size, sampling, scans=[(0,), (1,)]),
        'DQT behind the first SOS': write_multiscan(grids, size, sampling, dqt_late=True),
        'segment behind the third scan': write_multiscan(grids, size, sampling, tail=com),
        'fourth scan': write_multiscan(grids, size, sampling, scans=[(0,), (1,), (2,), (0,)]),
    }


def without_tables(coefs, size, sampling, omit=ALL_TABLES, qt=sc.QT, **kw):
    """The interleaved file coded with the Annex K tables and written without the DHT segments of `omit`."""
    lay = dict(kw.pop('layout', {}))
    lay['omit'] = tuple(omit)
    return sc.write(coefs, size, sampling, qt, layout=lay, **kw)


def scan_offsets(data):
    """[(first byte, one past the last)] of every scan's entropy-coded bytes in a writer file, in file order."""
    out = []
    i = 2
    while i < len(data):
        assert data[i] == 0xFF
        m = data[i + 1]
        if m == 0xD9:
            break
        L = (data[i + 2] << 8) | data[i + 3]
        i += 2 + L
        if m == 0xDA:
            j = i
            while not (data[j] == 0xFF and data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
            out.append((i, j))
            i = j
    return out
