"""NIfTI volumes -> the per-slice .npy directories CRCDataset and MICCAIBraTSDataset read (the reference's src/preprocess
scripts), with the arithmetic on the device: preprocess_crc.py, make_crc_testing_dataset.py, preprocess_brats.py."""
