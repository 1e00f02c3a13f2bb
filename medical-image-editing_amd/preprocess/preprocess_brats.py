"""BraTS patient directories -> the slice directory MICCAIBraTSDataset reads:
<dst>/<patient>/<patient>_<modality>_<%04d>.npy, modalities t1, t1ce, t2, flair (float32: z-score over the voxels > 0)
and seg (int32, nearest) - the reference's src/preprocess/preprocess_brats.py: np.rot90(k=3), resize to 256, and for a
source path that contains 'Training' the relabel 4 -> 3 of seg (a volume that already carries label 3 is an error).

    python preprocess/preprocess_brats.py --src <HGG dir> --src <LGG dir> --dst <dataset dir> [--image-size 256]

--src defaults to the environment variables TRAIN_HGG_SRC_PATH and TRAIN_LGG_SRC_PATH (those that are set), --dst to
TRAIN_BRATS_DST_PATH."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from preprocess.producers import DeviceProducer, is_scaled, resolve     # noqa: E402

IMAGE_SIZE = 256
MODALITIES = ('t1', 't1ce', 't2', 'flair', 'seg')


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="BraTS NIfTI volumes -> per-slice .npy dataset")
    parser.add_argument("--src", action="append", default=None, help="directory of patient directories; repeat for HGG and "
                        "LGG (default: $TRAIN_HGG_SRC_PATH and $TRAIN_LGG_SRC_PATH)")
    parser.add_argument("--dst", default=None, help="dataset directory to write (default: $TRAIN_BRATS_DST_PATH)")
    parser.add_argument("--image-size", type=int, default=IMAGE_SIZE)
    args = parser.parse_args(argv)
    if not args.src:
        args.src = [os.environ[k] for k in ("TRAIN_HGG_SRC_PATH", "TRAIN_LGG_SRC_PATH") if os.environ.get(k)]
        if not args.src:
            raise SystemExit("--src is not given and neither TRAIN_HGG_SRC_PATH nor TRAIN_LGG_SRC_PATH is set")
    args.dst = resolve(args.dst, "TRAIN_BRATS_DST_PATH", "--dst")
    return args


def preprocess(patient_id, src, dst, image_size, producer):
    """One patient: every modality's volume -> its slices.  Returns the number of files written."""
    from utils import nifti
    dst_patient_dir_path = os.path.join(dst, patient_id)
    os.makedirs(dst_patient_dir_path, exist_ok=True)
    n = 0
    for pattern in MODALITIES:
        raw, slope, inter, _ = nifti.load_raw(os.path.join(src, patient_id, patient_id + '_' + pattern + '.nii.gz'))
        if pattern == 'seg':
            if is_scaled(slope, inter):
                raw = raw.astype(np.float64) * (slope if slope != 0.0 else 1.0) + inter
            slices = producer.label_slices(raw.astype(np.int32), image_size, 'brats', 'Training' in src)
        else:
            slices = producer.image_slices(raw, slope, inter, image_size, 'zscore', 'brats')
        for i in range(slices.shape[0]):
            np.save(os.path.join(dst_patient_dir_path, patient_id + '_' + pattern + '_' + str(i).zfill(4) + '.npy'), slices[i])
        n += slices.shape[0]
    return n


def run(srcs, dst, image_size=IMAGE_SIZE, producer=None):
    """-> {patient id: files written}"""
    producer = producer or DeviceProducer()
    written = {}
    for src in srcs:
        for patient_id in sorted(os.listdir(src)):
            written[patient_id] = preprocess(patient_id, src, dst, image_size, producer)
    return written


def main(argv=None, producer=None):
    args = parse_args(argv)
    written = run(args.src, args.dst, args.image_size, producer)
    print("%d patients, %d files -> %s" % (len(written), sum(written.values()), args.dst))
    return written


if __name__ == '__main__':
    main()
