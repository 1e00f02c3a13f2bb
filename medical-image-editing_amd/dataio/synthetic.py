"""Synthetic slice dataset (`dataset_name: "synthetic"`, what the committed baseline configs name): the smooth random
fields of SURVEY.md §8(d) - a coarse Gaussian field, bilinearly enlarged, plus pixel noise, clamped to [-1, 1].

Every sample is a pure function of (seed, index): it is generated when asked for, from a generator seeded by the pair, so
any worker layout, sampler or resume point sees the same data.  Samples carry the keys of the file datasets
(`patient_id`, `slice_num`, `image`)."""
import torch
import torch.nn.functional as F
from torch.utils import data

SLICES_PER_PATIENT = 16
# distinct streams for the three splits of one run seed
_MODE_OFFSET = {'train': 0, 'val': 1, 'test': 2}


def synthetic_slice(seed, index, size):
    """-> (1, size, size) float32 in [-1, 1]."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(index)) % (2 ** 63 - 1))
    low_size = max(size // 8, 1)
    low = torch.randn(1, 1, low_size, low_size, generator=g)
    field = F.interpolate(low, size=(size, size), mode="bilinear", align_corners=False)
    return (field * 0.6 + 0.05 * torch.randn(1, 1, size, size, generator=g)).clamp_(-1, 1)[0]


class SyntheticSliceDataset(data.Dataset):
    def __init__(self, mode='train', image_size=256, n_samples=256, seed=0):
        super().__init__()
        assert mode in _MODE_OFFSET
        self.mode, self.image_size, self.n_samples = mode, int(image_size), int(n_samples)
        self.seed = int(seed) * 3 + _MODE_OFFSET[mode]

    def __len__(self):
        return self.n_samples

    def __getitem__(self, index):
        if not 0 <= index < self.n_samples:
            raise IndexError(index)
        return {'patient_id': 'synthetic_%s_%04d' % (self.mode, index // SLICES_PER_PATIENT),
                'slice_num': index % SLICES_PER_PATIENT, 'image': synthetic_slice(self.seed, index, self.image_size)}
