"""tests/test_gpu_find_motifs_iupac.py runs this in a process of its own with MCALLER_POISON=1, which the library reads once:
find_motifs --iupac of the files given, device against host statement, then the same without a control and with --all."""
import os
import sys


def main():
    from mcaller_amd import find_motifs as FM
    from mcaller_amd.device import get_device
    assert os.environ.get('MCALLER_POISON') == '1'
    ref, bed, control, shapes = sys.argv[1:5]
    for ctl, keep_all in ((control, False), (None, True)):
        n = FM.find_motifs(ref, bed, ctl, shapes=shapes, min_sites=1, keep_all=keep_all, out='host.tsv', iupac=True)
        counts = dict(FM.last_counts)
        assert FM.find_motifs_device(ref, bed, ctl, shapes=shapes, min_sites=1, keep_all=keep_all, out='device.tsv', iupac=True) == n
        assert FM.last_report == dict(by='device', reason=None, n_rows=n), FM.last_report
        assert open('device.tsv', 'rb').read() == open('host.tsv', 'rb').read() and n > 0
        ist = get_device().motif_report_iupac_last_stats()
        assert all(ist[name] == counts[name] for name in ('n_good', 'n_pure', 'n_maximal')), (ist, counts)
    print('iupac ok')


if __name__ == '__main__':
    main()
