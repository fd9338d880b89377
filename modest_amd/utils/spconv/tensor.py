"""``spconv.SparseConvTensor`` of spconv 1.2."""
import torch


class SparseConvTensor:
    """features (N, C) float32, indices (N, 4) int32 [b, z, y, x] with unique rows, spatial_shape [D, H, W].
    ``indice_dict`` maps an ``indice_key`` to the rulebook built under it and is shared by every tensor derived from
    this one; ``features`` is assignable (the backbones write ``out.features = bn(out.features)``)."""

    def __init__(self, features, indices, spatial_shape, batch_size, grid=None):
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(s) for s in spatial_shape]
        self.batch_size = int(batch_size)
        self.indice_dict = {}
        self.grid = grid

    @property
    def spatial_size(self):
        n = 1
        for s in self.spatial_shape:
            n *= s
        return n

    def find_indice_pair(self, key):
        if key is None:
            return None
        return self.indice_dict.get(key)

    def dense(self, channels_first=True):
        """(B, C, D, H, W), or (B, D, H, W, C): zeros where there is no site.  Plain indexing: autograd sees it."""
        idx = self.indices.long()
        out = self.features.new_zeros([self.batch_size, *self.spatial_shape, self.features.shape[1]])
        out[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = self.features
        if not channels_first:
            return out
        return out.permute(0, 4, 1, 2, 3).contiguous()

    @property
    def sparity(self):   # (sic: spconv's spelling)
        return self.indices.shape[0] / max(self.spatial_size * self.batch_size, 1)
