"""CRC volumes -> the training slice directory CRCDataset reads: <dst>/<patient>/<%04d>.npy, float32 in [0, 255]
(the reference's src/preprocess/preprocess_crc.py: min-max over the volume, img[::-1] then np.rot90, bilinear to 512).

    python preprocess/preprocess_crc.py --src <dir of *_image.nii.gz> --dst <dataset dir> [--image-size 512]

--src / --dst default to the environment variables SRC_CRC_DIR_PATH / DST_CRC_DIR_PATH."""
import argparse
import glob
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from preprocess.producers import DeviceProducer, resolve, write_crc_volume     # noqa: E402

IMAGE_SIZE = 512


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="CRC NIfTI volumes -> per-slice .npy dataset")
    parser.add_argument("--src", default=None, help="directory of *_image.nii.gz (default: $SRC_CRC_DIR_PATH)")
    parser.add_argument("--dst", default=None, help="dataset directory to write (default: $DST_CRC_DIR_PATH)")
    parser.add_argument("--image-size", type=int, default=IMAGE_SIZE)
    args = parser.parse_args(argv)
    args.src = resolve(args.src, "SRC_CRC_DIR_PATH", "--src")
    args.dst = resolve(args.dst, "DST_CRC_DIR_PATH", "--dst")
    return args


def run(src, dst, image_size=IMAGE_SIZE, producer=None):
    """-> {patient id: slice count}"""
    producer = producer or DeviceProducer()
    written = {}
    for image_file in sorted(glob.glob(os.path.join(src, '*_image.nii.gz'))):
        written[os.path.basename(image_file)] = write_crc_volume(image_file, dst, image_size, producer)
    return written


def main(argv=None, producer=None):
    args = parse_args(argv)
    written = run(args.src, args.dst, args.image_size, producer)
    print("%d volumes, %d slices -> %s" % (len(written), sum(written.values()), args.dst))
    return written


if __name__ == '__main__':
    main()
