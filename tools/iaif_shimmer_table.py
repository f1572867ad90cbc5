#!/usr/bin/env python3
"""The table of README "IAIF": the mean local shimmer of the 16 oracle vowels of tests/test_iaif_ref.py (-v a, gain 10,
pre-emphasis 1, F0 100, 22050 Hz; set shimmer 2, 5 and 10 %) on the flow and on the residual with vs_lpc's sets and with
IAIF's sets, per de-emphasis (0.95, 0.99, 1) and polarity (+1, -1).  CPU only: the restatements of tests/ (the device
gives the same sets bit for bit, tests/test_gpu_iaif.py).

    python tools/iaif_shimmer_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_iaif_ref import shimmer_table  # noqa: E402


def main():
    print("| set `-s` | on the flow | de-emphasis | polarity | residual, `vs_lpc` sets | residual, IAIF sets |")
    print("|---|---|---|---|---|---|")
    for S in (2, 5, 10):
        on_flow, table, ok = shimmer_table(S, (0.95, 0.99, 1.0))
        assert ok
        for (rho, pol), (lpc, iaif) in table.items():
            print("| %d | %.4f | %.2f | %+d | %.4f | %.4f |" % (S, on_flow, rho, pol, lpc, iaif))


if __name__ == "__main__":
    main()
