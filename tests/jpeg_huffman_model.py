"""A pure-Python model of the device Huffman decoder (csrc/jpeg_pack.h `lane_decode`, csrc/jpeg_huffman.hip), run on what
`vh.jpeg_pack` returns: subsequence states, rounds to a fixed point, prefix sum, write pass, DC pass, closing checks.  It documents the
algorithm and lets tests/test_jpeg_pack.py check it against the host decoder without a GPU.  Pure Python: fixture-sized frames only.

The state at a subsequence boundary is (bit position, block-in-MCU index c, zig-zag slot z).  Every block is 64 slots — end-of-block
jumps to 64 — so the slots consumed since the segment's start say which block, which component and which coefficient comes next."""
import numpy as np

import jpeg_synth

SUB_BITS = 1024
INVALID = None                 # "no valid state": never equal to a state


def tables_of(huff):
    """JPEG_HUFF_BYTES -> [component][0: DC, 1: AC] dicts of the HuffDev fields."""
    raw = np.asarray(huff, np.uint8).tobytes()
    out = []
    for k in range(6):
        b = raw[k * 1424:(k + 1) * 1424]
        out.append({"look": np.frombuffer(b, np.uint16, 512, 0), "maxcode": np.frombuffer(b, np.int32, 18, 1024), "valoff": np.frombuffer(b, np.int32, 17, 1096),
                    "nvals": int(np.frombuffer(b, np.int32, 1, 1164)[0]), "vals": np.frombuffer(b, np.uint8, 256, 1168)})
    return [out[0:2], out[2:4], out[4:6]]


def _symbol(win, t):
    """jpeg_entropy.h decode_symbol on a 32-bit window -> (symbol, code length) or None."""
    e = int(t["look"][win >> 23])
    if e:
        return e & 255, e >> 8
    code16 = win >> 16
    for length in range(10, 17):
        code = code16 >> (16 - length)
        if code <= int(t["maxcode"][length]):
            idx = code + int(t["valoff"][length])
            return (int(t["vals"][idx]), length) if 0 <= idx < t["nvals"] else None
    return None


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


class Frame:
    def __init__(self, packed):
        d = [int(v) for v in packed.desc]
        self.scan = bytes(np.asarray(packed.scan).tobytes()) + bytes(8)
        self.rows = np.asarray(packed.segments).tolist()
        self.tables = tables_of(packed.huff)
        self.comps, self.samp, self.mcus_x, self.blocks = d[4], (1 if d[4] == 1 else d[5]), d[6], d[12]
        self.bw = (d[8], d[10], d[10])
        self.first = (0, d[8] * d[9], d[8] * d[9] + d[10] * d[11])
        self.bpm = 1 if self.comps == 1 else self.samp * self.samp + 2

    def window(self, q):
        return (int.from_bytes(self.scan[q >> 3:(q >> 3) + 5], "big") >> (8 - (q & 7))) & 0xFFFFFFFF

    def component(self, c):
        return 0 if c < self.samp * self.samp else c - self.samp * self.samp + 1

    def block_of(self, index):
        """MCU-order block index -> index in the coefficient layout (per component, block raster)."""
        m, ci = divmod(index, self.bpm)
        y, x = divmod(m, self.mcus_x)
        comp, per = self.component(ci), (self.samp if ci < self.samp * self.samp else 1)
        j = ci if comp == 0 else 0
        return self.first[comp] + (y * per + j // per) * self.bw[comp] + x * per + j % per

    def lane(self, q0, qend_seg, entry, write=None):
        """One subsequence [q0, q0 + SUB_BITS) from ``entry`` = (bit offset, c, z) -> (exit state or INVALID, slots consumed).
        ``write`` = (coef, first block of the segment, slots before this subsequence, the segment's slot count, result dict): the write pass."""
        if entry is INVALID:
            return INVALID, 0
        q, c, z = q0 + entry[0], entry[1], entry[2]
        qend, slots = min(q0 + SUB_BITS, qend_seg), 0
        if write and write[2] >= write[3]:
            return INVALID, 0
        while q < qend:
            t = self.tables[self.component(c)]
            win = self.window(q)
            got = _symbol(win, t[0] if z == 0 else t[1])
            if got is None or (z == 0 and got[0] > 15):
                if write:
                    write[4]["status"] = "bad_dc_code" if z == 0 else "bad_ac_code"
                return INVALID, slots
            sym, length = got
            run, s = (0, sym) if z == 0 else (sym >> 4, sym & 15)
            value, at = 0, z + run
            if z == 0 or s:
                if at > 63:
                    if write:
                        write[4]["status"] = "zero_run_past_63"
                    return INVALID, slots
                if s:
                    value = _extend((win << length & 0xFFFFFFFF) >> (32 - s), s)
                znew = at + 1
            elif run == 15:
                znew = z + 16
                if znew > 64:
                    if write:
                        write[4]["status"] = "zero_run_past_63"
                    return INVALID, slots
            else:
                znew = 64                                        # end of block
            q += length + s
            if write:
                coef, first_block, before, seg_slots, res = write
                if q > qend_seg:
                    res["status"] = "data_ends_early"
                    return INVALID, slots
                if value:
                    coef[self.block_of(first_block + (before + slots) // 64), jpeg_synth.ZIGZAG[at]] = value
            slots += znew - z
            z = znew
            if z == 64:
                z, c = 0, (c + 1) % self.bpm
                if write and write[2] + slots >= write[3]:
                    write[4]["remaining"] = qend_seg - q
                    return INVALID, slots
        return (max(q - (q0 + SUB_BITS), 0), c, z), slots


def decode(packed):
    """-> (coefficients (blocks, 64) int16 in jpeg_entropy_decode's layout, status name, the most rounds a segment needed)."""
    f = Frame(packed)
    coef = np.zeros((f.blocks, 64), np.int16)
    status, most_rounds = "ok", 0
    nsubs = len(f.scan) // 128
    for s, (off, bitlen, mcu0, mcus) in enumerate(f.rows):
        sub0 = off // 128
        n = (f.rows[s + 1][0] // 128 if s + 1 < len(f.rows) else nsubs) - sub0
        qend = sub0 * SUB_BITS + bitlen
        start = (0, 0, 0)
        used = [start] * n                                       # the entry state each subsequence was last decoded from: the guess at first
        out = [f.lane((sub0 + i) * SUB_BITS, qend, start) for i in range(n)]
        for rounds in range(n + 1):                              # after round r the first r subsequences are exact
            entries = [start] + [o[0] for o in out[:-1]]
            again = [i for i in range(n) if entries[i] != used[i]]
            if not again:
                break
            for i in again:
                out[i], used[i] = f.lane((sub0 + i) * SUB_BITS, qend, entries[i]), entries[i]
        most_rounds = max(most_rounds, rounds)
        before, res = 0, {"status": "ok", "remaining": -1}
        for i in range(n):                                       # exclusive prefix sum of the slots + write pass
            f.lane((sub0 + i) * SUB_BITS, qend, start if i == 0 else out[i - 1][0], (coef, mcu0 * f.bpm, before, mcus * f.bpm * 64, res))
            before += out[i][1]
        if res["status"] == "ok":
            if res["remaining"] < 0:
                res["status"] = "blocks_short"
            elif s + 1 < len(f.rows) and res["remaining"] >= 8:
                res["status"] = "restart_marker_unread"
        if res["status"] != "ok" and status == "ok":
            status = res["status"]
        pred = [0, 0, 0]                                         # DC pass: running sum per component in MCU order, wrapping like int16
        for index in range(mcu0 * f.bpm, (mcu0 + mcus) * f.bpm):
            comp, blk = f.component(index % f.bpm), f.block_of(index)
            pred[comp] = (pred[comp] + int(coef[blk, 0])) & 0xFFFF
            coef[blk, 0] = np.uint16(pred[comp]).astype(np.int16)
    return coef, status, most_rounds
