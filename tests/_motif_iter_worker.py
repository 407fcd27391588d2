"""tests/test_gpu_find_motifs_iter.py runs this in a process of its own with MCALLER_POISON=1, which the library reads once:
find_motifs --iterative of the files given, device against host statement, rows and --unexplained file, in both modes, then the
same without a control and with --all."""
import os
import sys


def main():
    from mcaller_amd import find_motifs as FM
    from mcaller_amd.device import get_device
    assert os.environ.get('MCALLER_POISON') == '1'
    ref, bed, control, shapes = sys.argv[1:5]
    for ctl, keep_all in ((control, False), (None, True)):
        for iupac in (False, True):
            kw = dict(shapes=shapes, min_sites=3, keep_all=keep_all, iupac=iupac, iterative=True, max_motifs=6)
            n = FM.find_motifs(ref, bed, ctl, out='host.tsv', unexplained='host.bed', **kw)
            counts = dict(FM.last_counts)
            assert FM.find_motifs_device(ref, bed, ctl, out='device.tsv', unexplained='device.bed', **kw) == n
            assert FM.last_report == dict(by='device', reason=None, n_rows=n), FM.last_report
            assert open('device.tsv', 'rb').read() == open('host.tsv', 'rb').read() and n > 1
            assert open('device.bed', 'rb').read() == open('host.bed', 'rb').read()
            ist = get_device().motif_report_iter_last_stats()
            assert all(ist[name] == counts[name] for name in ('n_rounds', 'n_explained', 'n_unexplained')), (ist, counts)
    print('iterative ok')


if __name__ == '__main__':
    main()
