"""Hand-packed baseline JPEG streams: a grayscale 8x8 frame (one block, quantiser 1) whose Huffman tables are written here, so that a
test can give ANY symbol ANY code length — Pillow's encoder never gives a size-8 AC symbol a 1-bit code, a legal DHT may."""
import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _dht(cls, symbols_by_length):
    """symbols_by_length: {code length: [symbols]} -> the DHT payload and {symbol: code string} (canonical codes, T.81 Annex C)."""
    counts = [len(symbols_by_length.get(n, ())) for n in range(1, 17)]
    symbols = [s for n in range(1, 17) for s in symbols_by_length.get(n, ())]
    codes, code = {}, 0
    for n in range(1, 17):
        for s in symbols_by_length.get(n, ()):
            codes[s] = format(code, f"0{n}b")
            code += 1
        code <<= 1
    return bytes([cls << 4]) + bytes(counts) + bytes(symbols), codes


def _magnitude(v):
    """-> (size, bit string) of a non-zero coefficient (T.81 F.1.2.1: negative values as v - 1 in `size` bits)."""
    size = int(abs(v)).bit_length()
    return size, format(v if v > 0 else v + (1 << size) - 1, f"0{size}b")


def gray_block_stream(ac_by_length, coefficients):
    """One 8x8 grayscale block with DC 0: ``coefficients`` = [(zero run, value)] in zig-zag order, then EOB.  ``ac_by_length`` must
    hold every (run << 4 | size) symbol those need, and 0x00.  -> (bytes, the 64 expected coefficients in natural order)."""
    dc_payload, dc_codes = _dht(0, {1: [0]})
    ac_payload, ac_codes = _dht(1, ac_by_length)
    bits, k, want = dc_codes[0], 0, np.zeros(64, np.int16)
    for run, v in coefficients:
        size, mag = _magnitude(v)
        bits += ac_codes[(run << 4) | size] + mag
        k += run + 1
        want[ZIGZAG[k]] = v
    bits += ac_codes[0x00]
    bits += "1" * (-len(bits) % 8)
    scan = bytearray()
    for i in range(0, len(bits), 8):
        scan.append(int(bits[i:i + 8], 2))
        if scan[-1] == 0xFF:
            scan.append(0x00)
    data = (b"\xff\xd8" + _segment(0xDB, bytes([0]) + bytes([1] * 64)) + _segment(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0]))
            + _segment(0xC4, dc_payload) + _segment(0xC4, ac_payload) + _segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + bytes(scan) + b"\xff\xd9")
    return data, want


# A size-8 symbol on a 1-bit code (code + magnitude = 9 bits: as long as the decoder's look-ahead), size 7 on 3 bits, a run with size 7,
# and the values at both ends of each size.  Sum |c| / 4 < 512: inside the range libjpeg's sample range table and a clamp agree on.
SHORT_CODE_TABLE = {1: [0x08], 2: [0x00], 3: [0x07], 4: [0x17], 5: [0x09]}
SHORT_CODE_COEFFICIENTS = [(0, 200), (0, -200), (0, -128), (0, 255), (0, -255), (0, 100), (0, -64), (1, -127), (0, 127), (0, 128), (0, 256)]
