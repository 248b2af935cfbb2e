"""LDS bank-conflict check of every fragment read pattern the conv kernels use, under the bank model of
MI355X_MICROARCH.md (LDS): a wave64 access is serviced in fixed lane groups, one LDS cycle per group when no two lanes
of the group hit the same bank with different addresses; 64 banks x 4 B.
  ds_read_b128:        four groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32
  ds_read_b64_tr_b16:  two groups of 32 lanes
Prints LDS cycles per wave-instruction (ideal: 4 for b128, 2 for b64_tr).  CPU only; run it after touching a tile layout."""
G128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G128 = G128 + [[x + 32 for x in g] for g in G128]
G64 = [list(range(32)), list(range(32, 64))]


def cycles(addr, groups, nbytes):
    tot = 0
    for g in groups:
        banks = {}
        for l in g:
            a = addr(l)
            for d in range(nbytes // 4):
                banks.setdefault(((a // 4) + d) % 64, set()).add(a)
        tot += max(len(v) for v in banks.values())
    return tot


def igemm2_a(pitch, tx, k16):      # 32x32x16: lane = pixel l & 31, k half l >> 5
    return lambda l: ((l & 31) + tx) * pitch + (2 * k16 + (l >> 5)) * 16


def igemm2_b(pitch, tx, half):     # 16x16x32: lane = pixel l & 15, k quarter l >> 4
    return lambda l: ((l & 15) + 16 * half + tx) * pitch + (l >> 4) * 16


def igemm2_dma(m16, tx, sel):      # dense tile, chunk position = chunk ^ key(col)
    def f(l):
        if m16:
            col, chunk = (l & 15) + 16 * sel + tx, l >> 4
            return col * 64 + ((chunk ^ ((col >> 1) & 3)) * 16)
        col, chunk = (l & 31) + tx, 2 * sel + (l >> 5)
        return col * 64 + ((chunk ^ ((col >> 2) & 3)) * 16)
    return f


def wgrad2_tr(w16, swz, tx, h, second, LW=34, row=0):
    """transposed read of wgrad2: [pixel][64 B] rows.  32x32x16 form: pixel 8*(g4>>1) + (li>>2), channels 16*(g4&1) + 4*(li&3);
    16x16x32 form (W16): pixel 8*g4 + (li>>2), channels 16*h + 4*(li&3).  swz: the 32-B halves of a pixel whose tile column has
    bit 3 set are stored swapped."""
    def f(l):
        g4, li = l >> 4, l & 15
        if w16:
            col = tx + 8 * g4 + (li >> 2) + (4 if second else 0)
            half = h ^ (((col >> 3) & 1) if swz else 0)
            return (row * LW + col) * 64 + half * 32 + (4 * (li & 3)) * 2
        col = tx + 8 * (g4 >> 1) + (li >> 2) + (4 if second else 0) + 16 * h
        return (row * LW + col) * 64 + (16 * (g4 & 1) + 4 * (li & 3)) * 2
    return f


def fused_tr(pitch, col0, second):
    """transposed read of the fused backward (igemm2 FUSE, 32x32x16 form): pixel col0 + 8*(g4>>1) + (li>>2) (+ 4) of a tile row at
    `pitch` bytes per pixel -- 80 for the dY halo tile (col0 = 16 * half + 2 - tx), 64 for the interior x tile"""
    def f(l):
        g4, li = l >> 4, l & 15
        return (col0 + 8 * (g4 >> 1) + (li >> 2) + (4 if second else 0)) * pitch + (16 * (g4 & 1) + 4 * (li & 3)) * 2
    return f


if __name__ == "__main__":
    for pitch in (80, 96):
        a = [cycles(igemm2_a(pitch, tx, k), G128, 16) for tx in range(3) for k in range(2)]
        b = [cycles(igemm2_b(pitch, tx, h), G128, 16) for tx in range(3) for h in range(2)]
        print(f"igemm2 pitch {pitch}: 32x32x16 reads {a}  16x16x32 reads {b}")
    print("igemm2 DMA tiles: 32x32x16", [cycles(igemm2_dma(False, tx, k), G128, 16) for tx in range(3) for k in range(2)],
          " 16x16x32", [cycles(igemm2_dma(True, tx, h), G128, 16) for tx in range(3) for h in range(2)])
    for w16, swz in ((False, False), (True, False), (True, True)):
        r = [cycles(wgrad2_tr(w16, swz, tx, h, s, row=row), G64, 8) for tx in range(3) for h in range(2) for s in (False, True) for row in (0, 1)]
        print(f"wgrad2 transposed reads, 16x16x32={w16} swizzle={swz}: {r}")
    print("fused backward transposed reads: dY tile (80 B)", [cycles(fused_tr(80, 16 * h + 2 - tx, s), G64, 8) for tx in range(3) for h in range(2) for s in (False, True)],
          " x tile (64 B)", [cycles(fused_tr(64, 16 * h, s), G64, 8) for h in range(2) for s in (False, True)])
