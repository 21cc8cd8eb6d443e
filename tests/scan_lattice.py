"""The scan kernel's shape lattice as the tests use it: syzgydb_amd/scan_lattice.py builds it from the host-only plan hook
(one cell per lane-map class and per row-shape kernel, a small and a deep row count each).

`python tests/scan_lattice.py` prints the lattice.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from syzgydb_amd.scan_lattice import *  # noqa: E402,F401,F403
from syzgydb_amd.scan_lattice import main, scan_plan  # noqa: E402,F401

if __name__ == "__main__":
    main()
