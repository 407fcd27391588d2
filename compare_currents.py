#!/usr/bin/env python3
"""Entry point beside compare_genomes.py: `./compare_currents.py --native A.diffs.6 --control B.diffs.6`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.compare_currents import main

if __name__ == '__main__':
    main()
