#!/usr/bin/env python3
"""Entry point with the reference's name: `./compare_genomes.py --bed1 A.bed --bed2 B.bed`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.compare_genomes import main

if __name__ == '__main__':
    main()
