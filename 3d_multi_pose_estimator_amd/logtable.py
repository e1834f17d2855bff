"""The one table of logarithms behind the clustering scores: Engine.partition_scores hands it to the device
(mpe_set_log_table) and harness/partition.py reads it on the host, so both sides use the same numbers bit for bit."""
import numpy as np

from .lib import MPE_PART_MAX_SAMPLES

# the part the device is handed: every logarithm a frame of MPE_PART_MAX_SAMPLES labels can ask for
DEVICE_ENTRIES = MPE_PART_MAX_SAMPLES ** 2
_LOG = np.log(np.arange(1, DEVICE_ENTRIES + 1, dtype=np.float64))


def log_table(K=0):
    """log(1..K') as float64, K' >= max(K, DEVICE_ENTRIES); entry k - 1 is log k.  The table only ever grows at its end: an
    entry keeps its bits for the life of the process (what the device was handed stays what the host reads)."""
    global _LOG
    if K > len(_LOG):
        K = max(K, 2 * len(_LOG))
        _LOG = np.concatenate((_LOG, np.log(np.arange(len(_LOG) + 1, K + 1, dtype=np.float64))))
    return _LOG
