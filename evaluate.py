#!/usr/bin/env python3
"""Entry point: `./evaluate.py -f reads.eventalign.diffs.6 -p labelled_positions.txt [-d 15] [--depths 1,2,5]`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.evaluate import main

if __name__ == '__main__':
    main()
