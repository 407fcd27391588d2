#!/usr/bin/env python3
"""Entry point: `./motif_profile.py -r ref.fasta --bed SUMMARY.bed --motifs GATC:2,CCWGG:2 [--neighbours 5 --nn OUT.nn]`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mcaller_amd.motif_profile import main

if __name__ == '__main__':
    main()
