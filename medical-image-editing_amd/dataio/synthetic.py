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


LESION_EDGE = 2.0          # pixels over which a disc's profile falls from 1 to 0, centred on its radius


def synthetic_lesions(seed, index, size, n, radius, contrast):
    """-> (delta (1, size, size) float32, mask (1, size, size) uint8): n smooth-edged discs, a pure function of (seed, index) on a
    stream of its own (synthetic_slice's draws are not touched).  A disc's centre is uniform over the positions that keep it
    inside the slice, its radius uniform in [radius / 2, radius]; its profile is clamp((r - d) / LESION_EDGE + 0.5, 0, 1) of the
    distance d to the centre; delta = contrast * the largest profile at the pixel and mask = that profile >= 0.5 (d <= r)."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(index) + 7919 * 104729) % (2 ** 63 - 1))
    u = torch.rand(int(n), 3, generator=g, dtype=torch.float64)
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64), indexing="ij")
    profile = torch.zeros(size, size, dtype=torch.float64)
    for cy, cx, ur in u.tolist():
        r = float(radius) * (0.5 + 0.5 * ur)
        lo, hi = min(r, (size - 1) / 2.0), max(size - 1 - r, (size - 1) / 2.0)
        d = torch.sqrt((yy - (lo + cy * (hi - lo))) ** 2 + (xx - (lo + cx * (hi - lo))) ** 2)
        profile = torch.maximum(profile, ((r - d) / LESION_EDGE + 0.5).clamp_(0, 1))
    return (float(contrast) * profile).float()[None], (profile >= 0.5).to(torch.uint8)[None]


class SyntheticSliceDataset(data.Dataset):
    def __init__(self, mode='train', image_size=256, n_samples=256, seed=0, lesions=None):
        """lesions: None, or {'n', 'radius', 'contrast'} (a dict or an object with these attributes) - then every sample is the
        slice plus synthetic_lesions' delta, clamped to [-1, 1], and carries the mask as 'label'."""
        super().__init__()
        assert mode in _MODE_OFFSET
        self.mode, self.image_size, self.n_samples = mode, int(image_size), int(n_samples)
        self.seed = int(seed) * 3 + _MODE_OFFSET[mode]
        self.lesions = None
        if lesions is not None:
            get = lesions.get if isinstance(lesions, dict) else lambda k: getattr(lesions, k)
            self.lesions = (int(get('n')), float(get('radius')), float(get('contrast')))

    def __len__(self):
        return self.n_samples

    def __getitem__(self, index):
        if not 0 <= index < self.n_samples:
            raise IndexError(index)
        sample = {'patient_id': 'synthetic_%s_%04d' % (self.mode, index // SLICES_PER_PATIENT),
                  'slice_num': index % SLICES_PER_PATIENT, 'image': synthetic_slice(self.seed, index, self.image_size)}
        if self.lesions is not None:
            delta, mask = synthetic_lesions(self.seed, index, self.image_size, *self.lesions)
            sample['image'] = (sample['image'] + delta).clamp_(-1, 1)
            sample['label'] = mask
        return sample
