"""CRC volumes of the patients that are NOT in the training directory -> the held-out slice directory, in the layout of
preprocess_crc.py (the reference's src/preprocess/make_crc_testing_dataset.py).

    python preprocess/make_crc_testing_dataset.py --train <training dataset dir> --candidates <dir of *_image.nii.gz>
        --dst <dataset dir> [--image-size 512] [--expect-train-patients 289]

The directories default to the environment variables TRAIN_DATA_DIR_PATH / CANDIDATE_DIR_PATH / DIST_DIR_PATH.  The
reference asserts exactly 289 training patients; here that check is --expect-train-patients."""
import argparse
import glob
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from preprocess.producers import DeviceProducer, parse_patient_id, resolve, write_crc_volume     # noqa: E402

IMAGE_SIZE = 512


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="held-out CRC NIfTI volumes -> per-slice .npy dataset")
    parser.add_argument("--train", default=None, help="training dataset directory, one sub-directory per patient "
                        "(default: $TRAIN_DATA_DIR_PATH)")
    parser.add_argument("--candidates", default=None, help="directory of *_image.nii.gz (default: $CANDIDATE_DIR_PATH)")
    parser.add_argument("--dst", default=None, help="dataset directory to write (default: $DIST_DIR_PATH)")
    parser.add_argument("--image-size", type=int, default=IMAGE_SIZE)
    parser.add_argument("--expect-train-patients", type=int, default=None,
                        help="fail unless the training directory holds exactly this many patients")
    args = parser.parse_args(argv)
    args.train = resolve(args.train, "TRAIN_DATA_DIR_PATH", "--train")
    args.candidates = resolve(args.candidates, "CANDIDATE_DIR_PATH", "--candidates")
    args.dst = resolve(args.dst, "DIST_DIR_PATH", "--dst")
    return args


def run(train, candidates, dst, image_size=IMAGE_SIZE, expect_train_patients=None, producer=None):
    """-> {volume file name: slice count} of the patients written"""
    training_patients = os.listdir(train)
    if expect_train_patients is not None and len(training_patients) != expect_train_patients:
        raise SystemExit("%s holds %d patients, expected %d" % (train, len(training_patients), expect_train_patients))
    producer = producer or DeviceProducer()
    written = {}
    for image_file in sorted(glob.glob(os.path.join(candidates, '*_image.nii.gz'))):
        if parse_patient_id(image_file) not in training_patients:
            written[os.path.basename(image_file)] = write_crc_volume(image_file, dst, image_size, producer)
    return written


def main(argv=None, producer=None):
    args = parse_args(argv)
    written = run(args.train, args.candidates, args.dst, args.image_size, args.expect_train_patients, producer)
    print("%d volumes, %d slices -> %s" % (len(written), sum(written.values()), args.dst))
    return written


if __name__ == '__main__':
    main()
