"""The fixtures of the CABAC restore tests that restore_cases.py does not load (tests/golden/restore_cabac/*.npz; what each
holds: tests/golden/make_golden_cabac_cut.py and, for own_*.npz, tests/test_restore_cabac.py)."""
import os

import numpy as np

import golden_io

# The cli_*.npz set has no I-only CABAC stream: the reference's files of test_cif_I_CABAC_slice.264 are larger than a committed file may
# be.  Its first two pictures (14 slices each), as the reference wrote them, stand for it; the whole stream goes through the kernel in
# tests/test_restore_cabac_gpu.py
I_CUT = "cut_test_cif_I_CABAC_slice.264"
CONCAT = "concat_BA_MW_D.264+test_qcif_cabac.264"
# QCIF_2P_I_allIPCM.264 as lh264_compress_batch wrote it (the reference's files of it carry no I_PCM samples)
OWN_IPCM = "own_QCIF_2P_I_allIPCM.264"


def load(name):
    """(main, tags, the bytes that were compressed: those kept in the fixture, if any)"""
    z = np.load(os.path.join(golden_io.GOLDEN_DIR, "restore_cabac", name + ".npz"))
    return z["main"].tobytes(), {int(k[4:]): z[k].tobytes() for k in z.files if k.startswith("tag_")}, z["input"].tobytes() if "input" in z else None
