#!/usr/bin/env python3
"""Entry point beside compare_currents.py: `./cluster_sites.py -f reads.eventalign.diffs.6`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.cluster_sites import main

if __name__ == '__main__':
    main()
