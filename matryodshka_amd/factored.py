"""Factored high-res layer stacks: the inputs of `MSI.hres_layers` kept in place of the stack it builds.

A high-res stack carries no information beyond what it is computed from: texel (i, j) of layer d is a function of the two
preprocessed high-res images, the two composed poses, the source intrinsics and the align_corners resize of the low-res
blend_weights / alphas at (i, j).  A `FactoredLayers` holds exactly those pieces -- at 4096 x 2048 x 32 over a 640 x 320 network
254 MB, against 4.3 GB for the fp32 stack and 1.07 GB for `rgba8`, and nothing in it is quantised.  `MSI.hres_factors` makes one
(the checks, preprocessing and pose composition of `hres_layers`, no kernel of its own), `MSI.render_views` / `render_ods_pair`
render from it directly -- every output element compares == to the render of the fp32 stack, a zero may differ in sign --,
`MSI.materialize_layers` builds the stack (fp32, packed or sparse) for everything else, and `save` / `load` keep it in one `.npz`.

This module does not load the native library.
"""
import numpy as np
import torch

LAYOUT_VERSION = 1            # of the .npz written by FactoredLayers.save
_ARRAYS = ("blend_weights", "alphas", "ref_image", "src_image", "ref_pose", "src_pose", "intrinsics")


class FactoredLayers(object):
    """The factors of a high-res ODS layer stack (all fp32, contiguous, on one device).

    blend_weights, alphas   [B,h,w,D]: the low-res outputs of the network
    ref_image, src_image    [B,Hh,Wh,3]: the PREPROCESSED high-res images
    ref_pose, src_pose      [B,4,4]: the composed current poses (pose @ ref_pose_inv)
    intrinsics              [B,3,3]: the source intrinsics ([:, 0, 0] is the ODS baseline)
    planes                  the sphere radii (tuple of D floats, far -> near)
    shape                   (B, Hh, Wh, D): the [B,Hh,Wh,D,4] stack it stands for
    nbytes                  bytes of the seven arrays"""

    def __init__(self, blend_weights, alphas, ref_image, src_image, ref_pose, src_pose, intrinsics, planes):
        def f32(x):
            x = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            if x.dtype != torch.float32:
                raise ValueError("the factors are fp32, not %s" % (x.dtype,))
            return x.contiguous()
        bw, al, ref, src = f32(blend_weights), f32(alphas), f32(ref_image), f32(src_image)
        p0, p1, intr = f32(ref_pose), f32(src_pose), f32(intrinsics)
        if bw.dim() != 4 or bw.shape != al.shape:
            raise ValueError("blend_weights and alphas must be [B,h,w,D] and agree")
        b, d = bw.shape[0], bw.shape[3]
        if ref.dim() != 4 or ref.shape[0] != b or ref.shape[3] != 3 or src.shape != ref.shape:
            raise ValueError("ref_image and src_image must be [B,Hh,Wh,3], agree, and have the batch of blend_weights")
        if tuple(p0.shape) != (b, 4, 4) or tuple(p1.shape) != (b, 4, 4):
            raise ValueError("ref_pose and src_pose must be [B,4,4] = %s" % ((b, 4, 4),))
        if intr.numel() != b * 9:
            raise ValueError("intrinsics must be [B,3,3] with B = %d" % b)
        intr = intr.reshape(b, 3, 3)
        if len({t.device for t in (bw, al, ref, src, p0, p1, intr)}) != 1:
            raise ValueError("the factors must live on one device")
        if torch.is_tensor(planes):
            planes = planes.detach().cpu().reshape(-1).tolist()
        planes = tuple(float(p) for p in planes)
        if len(planes) != d:
            raise ValueError("len(planes) != number of layers")
        self.blend_weights, self.alphas, self.ref_image, self.src_image = bw, al, ref, src
        self.ref_pose, self.src_pose, self.intrinsics = p0, p1, intr
        self.planes = planes

    def _arrays(self):
        return tuple(getattr(self, name) for name in _ARRAYS)

    @property
    def device(self):
        return self.alphas.device

    @property
    def shape(self):
        return (self.alphas.shape[0], self.ref_image.shape[1], self.ref_image.shape[2], self.alphas.shape[3])

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._arrays())

    def to(self, device):
        return FactoredLayers(*(t.to(device) for t in self._arrays()), planes=self.planes)

    def save(self, path):
        """One .npz (no pickle): the seven arrays, planes, factored_layout_version."""
        with open(path, "wb") as f:
            np.savez(f, factored_layout_version=np.int64(LAYOUT_VERSION), planes=np.asarray(self.planes, np.float64),
                     **{name: t.cpu().numpy() for name, t in zip(_ARRAYS, self._arrays())})

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            if "factored_layout_version" not in z.files:
                raise ValueError("%s: not a FactoredLayers file (no factored_layout_version)" % path)
            version = int(z["factored_layout_version"])
            if version != LAYOUT_VERSION:
                raise ValueError("%s: factored layout version %d, this reader is written for %d" % (path, version, LAYOUT_VERSION))
            arrays = [z[name] for name in _ARRAYS]
            planes = tuple(z["planes"].tolist())
        for name, a in zip(_ARRAYS, arrays):
            if a.dtype != np.float32:
                raise ValueError("%s: %s stored as %s" % (path, name, a.dtype))
        out = cls(*arrays, planes=planes)
        return out if device is None else out.to(device)
