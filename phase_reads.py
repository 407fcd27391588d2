#!/usr/bin/env python3
"""Entry point beside compare_currents.py: `./phase_reads.py -f reads.diffs.6`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.phase_reads import main

if __name__ == '__main__':
    main()
