#!/usr/bin/env python3
"""Prints tfp_math.hpp's fin_table(): the 128 (invc, l10c) pairs of micro_of_coef_fast().

invc = 1 / (1 + (i + 0.5) / 128) rounded to a float (24 significant bits, so m * invc is exact in a
double for every 24-bit m), l10c = -10 log10(invc) of that rounded invc, correctly rounded to double
(mpmath at 200 bits). Also prints the split 10 log10(2) = K_HI + K_LO (K_HI: 45 significant bits)
and the Taylor coefficients (10 / ln 10) (-1)^(k+1) / k."""
import struct

import mpmath as mp

mp.mp.prec = 200


def f32(x):
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def main():
    print("  static constexpr FinEntry T[128] = {")
    for i in range(128):
        invc = f32(mp.mpf(1) / (1 + (mp.mpf(i) + mp.mpf(1) / 2) / 128))
        l10c = float(-10 * mp.log10(mp.mpf(invc)))
        end = "\n" if i % 2 else ""
        print(("      " if i % 2 == 0 else " ") + "{%s, %s}," % (float(invc).hex(), l10c.hex()), end=end)
    print("  };")
    k = 10 * mp.log10(2)
    hi = mp.ldexp(mp.floor(mp.ldexp(k, 43)), -43)  # k in [2, 4): 45 significant bits
    lo = float(k - hi)
    print("K_HI =", float(hi).hex(), " K_LO =", lo.hex())
    for n in range(1, 7):
        print("A%d =" % n, float((-1) ** (n + 1) * 10 / mp.log(10) / n).hex())


if __name__ == "__main__":
    main()
