#!/usr/bin/env python3
"""Entry point: `./find_motifs.py -r ref.fasta --bed SUMMARY.bed [--control CONTROL.bed]`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.find_motifs import main

if __name__ == '__main__':
    main()
