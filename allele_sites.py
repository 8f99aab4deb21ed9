#!/usr/bin/env python3
"""`python allele_sites.py -r ref.fa [-d DIR] [-o PREFIX] [--chrs a,b] [-R regions.bed] [-Q INT] [-G INT] [-g INT] [-J] [-n INT] [-F FRAC]
[-t INT] [-f] a.bam [b.bam ...]`: which base the reads of BAM file(s) carry where they disagree with the assembly --
`{DIR}/{PREFIX}.allele.{A,C,G,T}.depth.gz`, `.allele.sites.vcf`, `.allele.sites.bed` and `.allele.txt` -- from the BAM and FASTA bytes, by
the gfx950 HIP path in gci_amd/ -- see gci_amd/allelesites_cli.py.

Like GCI.py, a run imports no tensor library: its HBM buffers, streams and events are the library's own (gci_amd/hbm.py), and the
HIP runtime starts on a helper thread while the interpreter imports the rest."""
import os
import sys


def _wake_the_gpu():
    """The HIP runtime's own start on a thread of its own (see GCI.py); anything that goes wrong is left for the ordinary path."""
    try:
        import ctypes
        from gci_amd import _lib
        lib = _lib.load()
        n = ctypes.c_int(0)
        if lib.gci_dev_count(ctypes.byref(n)) == 0 and n.value > 0:
            lib.gci_dev_mem_info(0, None, None)
    except Exception:                                 # noqa: BLE001
        pass


_WAKER = None
if (__name__ == "__main__" and len(sys.argv) > 1 and not any(a in ("-h", "--help") for a in sys.argv[1:])
        and os.environ.get("GCI_HBM") != "torch" and os.environ.get("GCI_EARLY_HIP", "1") != "0"):
    import threading
    _WAKER = threading.Thread(target=_wake_the_gpu, daemon=True)
    _WAKER.start()

from gci_amd.allelesites_cli import main  # noqa: E402

if __name__ == "__main__":
    try:
        main(sys.argv)
    finally:
        if _WAKER is not None:
            _WAKER.join(timeout=10.0)
