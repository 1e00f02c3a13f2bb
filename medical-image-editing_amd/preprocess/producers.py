"""The slice producer the preprocess commands call, and what the three commands share.

A producer turns one volume into its slices:
    image_slices(raw, slope, inter, size, norm, orient) -> (Z, size, size) float32 numpy array
    label_slices(labels, size, orient, relabel)         -> (Z, size, size) int32 numpy array
with `raw` the (X, Y, Z) array of utils.nifti.load_raw in its stored dtype, `labels` an (X, Y, Z) int32 array, norm in
{'minmax', 'zscore', None} and orient in {'crc', 'brats', None} as hipops.ops.volume_to_slices takes them.  DeviceProducer
is the product path (one volume on the device at a time); the commands take another producer as a parameter so that file
layout and argument handling can be driven without a device.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# stored dtypes without a kernel of their own go up to the next one that holds every value
_WIDEN = {"int8": np.int16, "uint32": np.float64, "int64": np.float64, "uint64": np.float64}


class DeviceProducer:
    def __init__(self, device="cuda:0"):
        self.device = device

    def _upload(self, raw):
        import torch
        raw = np.asarray(raw)
        if raw.ndim != 3:
            raise ValueError("preprocess: expected a 3-D volume, got shape %s" % (raw.shape,))
        wide = _WIDEN.get(raw.dtype.name)
        if wide is not None:
            raw = raw.astype(wide)
        # (X, Y, Z) Fortran-ordered as the file holds it = (Z, Y, X) C-ordered: no copy on the host
        return torch.from_numpy(np.ascontiguousarray(raw.T)).to(self.device)

    def image_slices(self, raw, slope, inter, size, norm, orient):
        from hipops import ops
        vol = self._upload(raw)
        return ops.volume_to_slices(vol, size, norm=norm, orient=orient, slope=slope, inter=inter).cpu().numpy()

    def label_slices(self, labels, size, orient, relabel):
        from hipops import ops
        vol = self._upload(np.asarray(labels, dtype=np.int32))
        return ops.label_volume_to_slices(vol, size, orient=orient, relabel=relabel).cpu().numpy()


def is_scaled(slope, inter):
    """Whether nibabel would apply scl_slope / scl_inter (a slope of 0 means 'not set')."""
    return slope not in (0.0, 1.0) or inter != 0.0


def parse_patient_id(file_path):
    """'<a>_<b>_image.nii.gz' -> '<a>_<b>': the first two '_'-separated fields of the file name."""
    return '_'.join(os.path.basename(file_path).split('_')[:2])


def resolve(value, env_name, flag):
    """An argument, else the environment variable the reference read through dotenv."""
    if value:
        return value
    value = os.environ.get(env_name)
    if not value:
        raise SystemExit("%s is not given and %s is not set" % (flag, env_name))
    return value


def write_crc_volume(image_file, dst_root, image_size, producer):
    """One CRC volume -> <dst_root>/<patient>/<%04d>.npy (float32, min-max to [0, 255]).  Returns the slice count."""
    from utils import nifti
    raw, slope, inter, _ = nifti.load_raw(image_file)
    slices = producer.image_slices(raw, slope, inter, image_size, 'minmax', 'crc')
    save_dir_path = os.path.join(dst_root, parse_patient_id(image_file))
    os.makedirs(save_dir_path, exist_ok=True)
    for i in range(slices.shape[0]):
        np.save(os.path.join(save_dir_path, str(i).zfill(4) + '.npy'), slices[i])
    return slices.shape[0]
