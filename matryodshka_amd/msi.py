"""MI355X-native counterpart of the reference's `matryodshka.msi.MSI` class for the
infer -> render hot path, with the reference's method names and argument order
(so it drops into a test.py-style harness, test.py:127-159).

All arithmetic runs in libmsi_hip.so (hand-written HIP for gfx950) through the C
ABI of include/msi_hip.h; torch is used for device memory, streams and tiny 4x4
pose algebra only.  There is no CPU path: tensors must live on a HIP device.

Differences from the reference that are forced by leaving TF graph mode:
  * hidden graph inputs (`ref_pose_inv:0`, msi.py:1115) are keyword arguments with
    the test.py defaults (ref_pose_inv = inverse(ref_pose), no jitter);
  * global FLAGS become constructor arguments (coord_net);
  * batch semantics: the reference only works for B=1 (test.py:89, msi.py:1109);
    here B frames are B independent B=1 evaluations;
  * `rgba_layers` keeps the public [B,H,W,D,4] shape but is a permuted VIEW of the
    D-major [B,D,H,W,4] stack the kernels use (the layout msi.py:422 transposes to).
"""
import numpy as np
import torch

from . import _native as N
from . import nets
from .factored import FactoredLayers
from .mips import MipLayers, check_levels as check_mip_levels, level_shapes as mip_level_shapes, max_levels as max_mip_levels
from .packed import FORMATS as PACKED_FORMATS, PackedLayers
from .sparse import BORDERS, SparseLayers, TILE_H, TILE_W


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _on_own_device(cls):
    """Every public method runs with the model's device current: the native library launches on the stream it is
    handed, plans read the CU count of the current device, and per-device kernel attributes are set on first use --
    a caller driving several GPUs from one thread must not have to remember torch.cuda.set_device."""
    import functools

    def wrap(fn):
        @functools.wraps(fn)
        def inner(self, *args, **kwargs):
            if torch.cuda.current_device() == self.device.index:
                return fn(self, *args, **kwargs)
            with torch.cuda.device(self.device):
                return fn(self, *args, **kwargs)
        return inner

    inner = ("inv_depths", "_depths", "_current_poses", "_net_input", "_net_plan")     # no device work, or only ever called from a wrapped method
    for name, fn in list(vars(cls).items()):
        if callable(fn) and not name.startswith("__") and not isinstance(fn, (staticmethod, classmethod)) and name not in inner:
            setattr(cls, name, wrap(fn))
    return cls


@_on_own_device
class MSI(object):
    """Class definition for the MSI inference module (reference: msi.py:33-38)."""

    COLOR_SCHEMES = {'blend_psv': 0, 'blend_bg': 1, 'blend_bg_psv': 2, 'alpha_only': 3}   # MSI_COLOR_* of msi_hip.h

    def __init__(self, weights=None, coord_net=None, device=None, input_type='ODS', dtype='f32'):
        """coord_net: FLAGS.coord_net (test.py:52, default False = msi_train_net; the released ODS models are run with
        --coord_net = msi_coord_train_net, scripts/test/ods-wotemp-elpips-coord-reg.sh).  None (default): taken from the
        weights -- CoordNet's conv1_1/weights carry one extra input channel (nets.py:260-270), and the sweep volume's
        6 D channels are even -- or False without weights."""
        if not torch.cuda.is_available():
            raise RuntimeError("matryodshka_amd.MSI needs a HIP device (no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._coord_explicit = coord_net is not None
        self.coord_net = bool(coord_net)
        if input_type not in ('ODS', 'PP'):
            raise ValueError("input_type must be 'ODS' or 'PP' (FLAGS.input_type, msi.py:1157-1161)")
        self.input_type = input_type
        # 'bf16' = BASELINE configs[2] (and its PP counterpart): the sweep volume, the weights and the activations of the
        # network are bf16 (fp32 accumulate, fp32 LayerNorm statistics, fp32 prediction); geometry stays fp32
        if dtype not in ('f32', 'bf16'):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        self.dtype = dtype
        self._weights = None
        self._blob_cache = {}     # (in_channels, num_outputs, ngf) -> np blob
        self._packed_cache = {}   # desc key -> device tensor
        self._ws_cache = {}       # desc key -> (native plan, device workspace)
        self.net_options = {}     # msi_net_plan_set_option key -> value, applied to plans created from now on (tests)
        self._trig_cache = {}     # (H, W) -> device tensor
        self._planes_cache = {}   # tuple(planes) -> device tensor
        self._render_status = torch.zeros(1, dtype=torch.int32, device=self.device)   # msi_render_*'s status_device word
        if weights is not None:
            self.load_weights(weights)

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _f32(self, x):
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, dtype=np.float32))
        return x.to(device=self.device, dtype=torch.float32).contiguous()

    def _trig(self, height, width):
        key = (height, width)
        t = self._trig_cache.get(key)
        if t is None:
            host = np.empty(N.lib.msi_trig_table_floats(height, width), dtype=np.float32)
            N.check(N.lib.msi_build_trig_tables_host(height, width, host.ctypes.data), "msi_build_trig_tables_host")
            t = torch.from_numpy(host).to(self.device)
            self._trig_cache[key] = t
        return t

    def _planes(self, planes):
        if torch.is_tensor(planes):
            return planes.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        key = tuple(float(p) for p in planes)
        t = self._planes_cache.get(key)
        if t is None:
            t = torch.tensor(key, dtype=torch.float32).to(self.device)
            self._planes_cache[key] = t
        return t

    def _depths(self, planes, d):
        """The planes of a stack of d layers on the device."""
        depths = self._planes(planes)
        if depths.numel() != d:
            raise ValueError("len(planes) != number of layers")
        return depths

    def _current_poses(self, ref_pose, src_pose, ref_pose_inv, b, jitter_pose_inv=None):
        """curr_pose = pose @ ref_pose_inv of the reference and the source image, [2,B,4,4], in one launch (msi.py:1125); a missing
        ref_pose_inv is computed on the host (pass it explicitly to avoid the round trip); jitter: msi.py:1120."""
        if ref_pose_inv is None:
            ref_pose_inv = torch.linalg.inv(torch.as_tensor(ref_pose, dtype=torch.float32).cpu().double()).float()   # test.py:111
        ref_pose, src_pose, ref_pose_inv = self._f32(ref_pose), self._f32(src_pose), self._f32(ref_pose_inv)
        if jitter_pose_inv is not None:
            ref_pose_inv = self._compose(ref_pose_inv, jitter_pose_inv)
        if ref_pose_inv.shape[0] != b:
            ref_pose_inv = ref_pose_inv.reshape(-1, 4, 4).expand(b, 4, 4).contiguous()
        cur = torch.empty((2, b, 4, 4), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_compose_pose_pair_f32(ref_pose.data_ptr(), src_pose.data_ptr(), ref_pose_inv.data_ptr(),
                                                cur[0].data_ptr(), cur[1].data_ptr(), b, self._stream()),
                "msi_compose_pose_pair_f32")
        return cur

    def load_weights(self, weights):
        """weights: dict TF-variable-name -> array (see nets.variable_shapes)."""
        try:
            cin_w = int(nets._lookup(weights, "conv1_1/weights").shape[2])
        except (KeyError, AttributeError, IndexError):
            cin_w = None
        if cin_w is not None:
            has_coord = cin_w % 2 == 1            # 6 D sweep channels (+ 1 for CoordNet's |sin(lat)| channel)
            if not self._coord_explicit:
                self.coord_net = has_coord
            elif has_coord != self.coord_net:
                raise ValueError("MSI(coord_net=%s) but conv1_1/weights has %d input channels: these are %s weights"
                                 % (self.coord_net, cin_w, "CoordNet (msi_coord_train_net)" if has_coord else "msi_train_net"))
        self._weights = weights
        self._blob_cache.clear()
        self._packed_cache.clear()

    def _net_plan(self, batch, height, width, in_channels, num_outputs, ngf):
        """(descriptor, packed weights, workspace, plan) of a network shape, each made once and cached."""
        if self._weights is None:
            raise RuntimeError("MSI: no network weights loaded (load_weights / weights=...)")
        key = (batch, height, width, in_channels, num_outputs, ngf, self.coord_net, self.dtype)
        desc = nets.make_desc(batch, height, width, in_channels, num_outputs, ngf, self.coord_net, self.dtype)
        pkey = key[1:]  # packing does not depend on the batch size
        packed = self._packed_cache.get(pkey)
        if packed is None:
            bkey = (in_channels, num_outputs, ngf)
            blob = self._blob_cache.get(bkey)
            if blob is None:
                blob = nets.flatten_params(self._weights, in_channels, num_outputs, ngf, self.coord_net)
                self._blob_cache[bkey] = blob
            packed = torch.from_numpy(nets.pack_params(desc, blob)).to(self.device)
            self._packed_cache[pkey] = packed
        key = key + tuple(sorted(self.net_options.items()))
        pw = self._ws_cache.get(key)
        if pw is None:
            plan = N.NetPlan(desc, self.net_options)      # layer table, tiling and work split resolved once
            ws = torch.empty(plan.workspace_bytes(), dtype=torch.uint8, device=self.device)
            pw = (plan, ws)
            self._ws_cache[key] = pw
        return desc, packed, pw[1], pw[0]

    def _net(self, *shape):          # (what tests and tools unpack: descriptor, packed weights, workspace)
        return self._net_plan(*shape)[:3]

    def _plan(self, *shape):
        return self._net_plan(*shape)[3]

    def _net_input(self, net_input):
        """net_input as the plans of this model read it: contiguous, bf16 for a bf16 model."""
        want = torch.bfloat16 if self.dtype == 'bf16' else torch.float32
        if net_input.dtype != want or not net_input.is_contiguous():
            net_input = net_input.to(want).contiguous()
        return net_input

    def network_status(self):
        """msi_net_plan_status of the LAST network forward of this model: raises MsiError (MSI_E_RANGE) when a LayerNorm
        statistic left the fixed-point window the kernels resolve (mis-scaled or non-finite input; see include/msi_hip.h).
        Synchronises the stream -- call it after a frame, not inside a timed loop.  Returns the status bits (0)."""
        if getattr(self, "_last_forward", None) is None:
            return 0
        plan, ws = self._last_forward
        bits = N.c_int32(0)
        N.check(N.lib.msi_net_plan_status(plan.handle, ws.data_ptr(), self._stream(), N.ctypes.byref(bits)), "msi_net_plan_status")
        return int(bits.value)

    def calibrate(self, net_input, num_outputs=None, ngf=64):
        """msi_net_plan_calibrate: centre every layer's LayerNorm fixed-point window on the raw output this network really produces for `net_input`
        ([B,H,W,Cin], the forward's layout; a representative frame).  The packer derives the windows from the weights alone; a checkpoint whose trained
        gamma / beta / weights break that estimate makes network_status() raise MSI_E_RANGE on every frame -- call this once (the harness does, on the
        first flagged sample) and the windows follow the measurement.  The packed blob is modified in place on the device: every plan of this model
        (any batch size) uses the new windows.  Blocking; returns the number of layers whose window moved.  All or nothing: when it raises (MSI_E_RANGE: a layer
        without finite, non-constant output on this frame) the windows are exactly what they were before the call."""
        b, h, w, cin = net_input.shape
        if num_outputs is None:
            num_outputs = cin // 3          # blend_psv: 6 D -> 2 D
        _, packed, ws, plan = self._net_plan(b, h, w, cin, num_outputs, ngf)
        net_input = self._net_input(net_input)
        changed = N.c_int32(0)
        N.check(N.lib.msi_net_plan_calibrate(plan.handle, packed.data_ptr(), net_input.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(),
                                             N.ctypes.byref(changed)), "msi_net_plan_calibrate")
        return int(changed.value)

    def render_status(self):
        """Status word of the renders since the last call (include/msi_hip.h: MSI_RENDER_STATUS_*): raises ValueError when a
        ray origin -- handed over in DEVICE memory, where the host-side guard cannot look without a sync -- was not inside
        the innermost sphere (the kernel clamped the discriminant: finite pixels, not reference-defined).  Synchronises the
        stream -- call it after a frame, not inside a timed loop -- and resets the word.  Returns 0."""
        bits = int(self._render_status.item())
        if bits:
            self._render_status.zero_()
        if bits & N.RENDER_STATUS_ORIGIN_OUTSIDE:
            raise ValueError("a render's ray origin (pose @ tgt_pos) was not inside the innermost sphere: the reference takes "
                             "sqrt of a negative number there (spherical.py:316-318); the pixels of that call are not defined")
        return bits

    # ------------------------------------------------------------------ msi.py:1196-1217
    def inv_depths(self, start_depth, end_depth, num_depths):
        """num_depths sphere radii uniform in inverse depth, both ends included exactly, far -> near
        (python floats, fp64; tests assert equality with the oracle's restatement of msi.py:1196-1217)."""
        near, far = float(start_depth), float(end_depth)
        n = int(num_depths)
        lo, hi = 1.0 / near, 1.0 / far
        radii = [near, far] + [1.0 / (lo + (hi - lo) * (float(k) / float(n - 1))) for k in range(1, n - 1)]
        return sorted(radii, reverse=True)

    # ------------------------------------------------------------------ msi.py:1163-1194
    def preprocess_image(self, image):
        """uint8 [0,255] or float [0,1] -> float [-1,1] (msi.py:1163-1171)."""
        if not torch.is_tensor(image):
            image = torch.as_tensor(np.asarray(image))
        image = image.to(self.device).contiguous()
        out = torch.empty(image.shape, dtype=torch.float32, device=self.device)
        if image.dtype == torch.uint8:
            N.check(N.lib.msi_preprocess_u8_f32(image.data_ptr(), out.data_ptr(), image.numel(), self._stream()),
                    "msi_preprocess_u8_f32")
        else:
            image = image.to(torch.float32)
            N.check(N.lib.msi_preprocess_f32(image.data_ptr(), out.data_ptr(), image.numel(), self._stream()),
                    "msi_preprocess_f32")
        return out

    def preprocess_image_pair(self, image0, image1):
        """preprocess_image of two uint8 images of one shape in a single launch (raw_src_image / raw_ref_image)."""
        if not (torch.is_tensor(image0) and torch.is_tensor(image1) and image0.dtype == torch.uint8 and
                image1.dtype == torch.uint8 and image0.shape == image1.shape):
            return self.preprocess_image(image0), self.preprocess_image(image1)
        image0, image1 = image0.to(self.device).contiguous(), image1.to(self.device).contiguous()
        out = torch.empty((2,) + tuple(image0.shape), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_preprocess_pair_u8_f32(image0.data_ptr(), image1.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                 image0.numel(), self._stream()), "msi_preprocess_pair_u8_f32")
        return out[0], out[1]

    def deprocess_image_and_depth(self, rgb, depth):
        """deprocess_image(rgb), deprocess_depth_image(depth) (test.py:149-159) in a single launch."""
        rgb, depth = self._f32(rgb), self._f32(depth)
        if rgb.shape != depth.shape:
            return self.deprocess_image(rgb), self.deprocess_depth_image(depth)
        out = torch.empty((2,) + tuple(rgb.shape), dtype=torch.uint8, device=self.device)
        N.check(N.lib.msi_deprocess_pair_f32_u8(rgb.data_ptr(), depth.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                rgb.numel(), self._stream()), "msi_deprocess_pair_f32_u8")
        return out[0], out[1]

    def _deprocess(self, image, is_depth):
        image = self._f32(image)
        out = torch.empty(image.shape, dtype=torch.uint8, device=self.device)
        N.check(N.lib.msi_deprocess_f32_u8(image.data_ptr(), out.data_ptr(), image.numel(), is_depth, self._stream()),
                "msi_deprocess_f32_u8")
        return out

    def deprocess_image(self, image):
        """float [-1,1] -> uint8 (msi.py:1173-1181)."""
        return self._deprocess(image, 0)

    def deprocess_depth_image(self, image):
        """float [0,1] -> uint8 without the (x+1)/2 (msi.py:1186-1194)."""
        return self._deprocess(image, 1)

    def _compose(self, lhs, rhs):
        """[B,4,4] @ [B,4,4] on the device (msi_compose_poses_f32)."""
        lhs, rhs = self._f32(lhs), self._f32(rhs)
        if lhs.dim() == 2:
            lhs = lhs[None]
        if rhs.dim() == 2:
            rhs = rhs[None]
        if rhs.shape[0] != lhs.shape[0]:
            rhs = rhs.expand(lhs.shape[0], 4, 4).contiguous()
        out = torch.empty((lhs.shape[0], 4, 4), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_compose_poses_f32(lhs.data_ptr(), rhs.data_ptr(), out.data_ptr(), lhs.shape[0], self._stream()),
                "msi_compose_poses_f32")
        return out

    # ------------------------------------------------------------------ msi.py:1094-1130
    def format_network_input(self, ref_image, src_image, ref_pose, src_pose, planes, intrinsics,
                             ref_pose_inv=None, jitter_pose_inv=None, dtype=None):
        """Format the network input into the double sphere-sweep volume.
        Returns net_input [B,H,W,2*3*len(planes)].
        jitter_pose_inv: the hidden graph input `jitter_pose_inv:0` of FLAGS.jitter (msi.py:1118-1120):
        ref_pose_inv <- ref_pose_inv @ jitter_pose_inv.  dtype: 'f32' forces an fp32 volume on a bf16 model."""
        ref_image = self._f32(ref_image)
        src_image = self._f32(src_image)
        b, h, w, c = ref_image.shape
        if c != 3 or src_image.shape != ref_image.shape:
            raise ValueError("format_network_input: images must be [B,H,W,3] and agree")
        cur = self._current_poses(ref_pose, src_pose, ref_pose_inv, b, jitter_pose_inv)
        depths = self._planes(planes)
        nd = depths.numel()
        intr = self._f32(intrinsics)
        trig = self._trig(h, w)
        bf16 = (dtype or self.dtype) == 'bf16'
        psv = torch.empty((b, h, w, 6 * nd), dtype=torch.bfloat16 if bf16 else torch.float32, device=self.device)
        # order = +1 for the reference image (i = 0), -1 for the source (i = 1), msi.py:1127
        if self.input_type == 'ODS':
            N.check(N.lib.msi_ods_sweep_volume(ref_image.data_ptr(), src_image.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(),
                                               intr.data_ptr(), depths.data_ptr(), trig.data_ptr(), b, h, w, nd,
                                               psv.data_ptr(), 1 if bf16 else 0, self._stream()), "msi_ods_sweep_volume")
        elif bf16:   # sweep_src for perspective inputs (msi.py:1157-1161), the whole bf16 volume in one launch
            N.check(N.lib.msi_perspective_sweep_volume_bf16(ref_image.data_ptr(), src_image.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(),
                                                            intr.data_ptr(), depths.data_ptr(), b, h, w, nd, psv.data_ptr(), self._stream()),
                    "msi_perspective_sweep_volume_bf16")
        else:   # sweep_src for perspective inputs (msi.py:1157-1161); ref_pose_inv = interp_pose_inv (:1113)
            for i, img in enumerate((ref_image, src_image)):
                N.check(N.lib.msi_perspective_plane_sweep_f32(
                    img.data_ptr(), cur[i].data_ptr(), intr.data_ptr(), depths.data_ptr(),
                    b, h, w, nd, psv.data_ptr(), 6 * nd, i * 3 * nd, self._stream()),
                    "msi_perspective_plane_sweep_f32")
        return psv

    # ------------------------------------------------------------------ msi.py:40-289
    def infer_msi(self, raw_src_image, raw_ref_image, raw_hres_src_image, raw_hres_ref_image,
                  ref_pose, src_pose, intrinsics, which_color_pred, num_msi_planes, psv_planes,
                  extra_outputs='', ngf=64, ref_pose_inv=None, jitter_pose_inv=None, layer_format='f32'):
        """Construct and run the MSI inference path.  Returns (pred dict, net_input).
        Note the reference's argument order: src before ref (msi.py:40-46).
        which_color_pred: blend_psv (2D outputs) | blend_bg (2D+3) | blend_bg_psv (3D+3) | alpha_only (D), msi.py:119-275.
        layer_format: see infer_layers; a packed stack (pred['packed_layers']) carries psv_planes as its planes."""
        if which_color_pred not in self.COLOR_SCHEMES:
            raise ValueError("which_color_pred=%r (blend_psv, blend_bg, blend_bg_psv, alpha_only)" % which_color_pred)
        if len(psv_planes) != num_msi_planes:
            # msi.py:138 indexes the src PSV with num_msi_planes
            raise ValueError("infer_msi assumes len(psv_planes) == num_msi_planes (msi.py:138)")
        src_image, ref_image = self.preprocess_image_pair(raw_src_image, raw_ref_image)
        net_input = self.format_network_input(ref_image, src_image, ref_pose, src_pose, psv_planes,
                                              intrinsics, ref_pose_inv=ref_pose_inv, jitter_pose_inv=jitter_pose_inv)
        pred = self.infer_layers(net_input, num_msi_planes, ngf, extra_outputs, which_color_pred, layer_format=layer_format)
        return self._carrying(pred, psv_planes), net_input

    @staticmethod
    def _carrying(pred, planes):
        """pred with `planes` attached to its PackedLayers, where it has one."""
        if 'packed_layers' in pred:
            pk = pred['packed_layers']
            pred['packed_layers'] = PackedLayers(pk.data, pk.format, planes)
        return pred

    def run_net(self, net_input, num_outputs, ngf=64):
        """msi_net(net_input, num_outputs) (msi.py:95-125): [B,H,W,Cin] -> [B,H,W,num_outputs]."""
        b, h, w, cin = net_input.shape
        _, packed, ws, plan = self._net_plan(b, h, w, cin, num_outputs, ngf)
        net_input = self._net_input(net_input)
        pred = torch.empty((b, h, w, num_outputs), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_net_plan_forward(plan.handle, packed.data_ptr(), net_input.data_ptr(), pred.data_ptr(),
                                           ws.data_ptr(), ws.numel(), self._stream()), "msi_net_plan_forward")
        self._last_forward = (plan, ws)
        return pred

    @staticmethod
    def _layer_formats(layer_format):
        """layer_format of infer_layers -> (want the fp32 stack, packed format or None)."""
        allowed = ('f32',) + PACKED_FORMATS
        req = (layer_format,) if isinstance(layer_format, str) else tuple(layer_format) if isinstance(layer_format, (tuple, list)) else None
        if not req or any(not isinstance(f, str) or f not in allowed for f in req):
            raise ValueError("layer_format must be one of %s or a tuple of them, not %r" % (allowed, layer_format))
        packed = sorted(set(f for f in req if f != 'f32'))
        if len(packed) > 1:
            raise ValueError("layer_format takes at most one packed format per call (%s: 'f32' plus one of %s), not %r"
                             % (allowed, PACKED_FORMATS, layer_format))
        return 'f32' in req, (packed[0] if packed else None)

    def infer_layers(self, net_input, num_msi_planes, ngf=64, extra_outputs='', which_color_pred='blend_psv',
                     event_after_convs=None, layer_format='f32'):
        """msi_net + layer_prediction of infer_msi (msi.py:95-147): net_input -> pred dict.  For the reference's default
        colour scheme the 1x1 head, conv8_2's LayerNorm and the RGBA assembly run as ONE fused kernel
        (msi_net_plan_forward_rgba: the tanh prediction never goes to HBM; fp32: bit-identical to the two-step path,
        bf16: the same bf16 operands, fp32 summation order of the head differs);
        everything else takes run_net + assemble_layers.  event_after_convs: torch.cuda.Event (already recorded once, so
        that its handle exists) recorded between the convolutions and the fused tail.
        layer_format: 'f32' (default), 'rgba8', 'rgba16f', or a tuple of them with at most one packed format.  'f32' in the
        request -> pred['rgba_layers']; a packed format -> pred['packed_layers'], a PackedLayers (native layout, no planes
        attached) that the fused kernel writes itself (msi_net_plan_forward_layers: bit-identical to pack_layers of the fp32
        stack, which a packed-only request never allocates).  Where the fused tail does not apply the packed stack is
        pack_layers of the assembled fp32 one: the same bits for every configuration."""
        want_f32, pfmt = self._layer_formats(layer_format)
        b, h, w, cin = net_input.shape
        d = num_msi_planes
        fused = (which_color_pred == 'blend_psv' and
                 net_input.dtype == (torch.float32 if self.dtype == 'f32' else torch.bfloat16) and
                 cin == 6 * d and d % 4 == 0 and d <= 64 and ngf <= 64 and
                 (d <= 32 or d % (8 if self.dtype == 'f32' else 16) == 0) and    # D > 32: two layer groups of whole vectors
                 self.net_options.get(N.NET_OPT_HEAD_FUSE_LN, 1) and net_input.is_contiguous())
        if not fused:
            num_outputs = {'blend_psv': 2 * d, 'blend_bg': 2 * d + 3, 'blend_bg_psv': 3 * d + 3, 'alpha_only': d}[which_color_pred]
            msi_pred = self.run_net(net_input, num_outputs, ngf)
            if event_after_convs is not None:
                event_after_convs.record()
            pred = self.assemble_layers(net_input, msi_pred, d, extra_outputs, which_color_pred)
            if pfmt is not None:
                pred['packed_layers'] = self.pack_layers(pred['rgba_layers'], pfmt)
                if not want_f32:
                    del pred['rgba_layers']
            return pred
        _, packed, ws, plan = self._net_plan(b, h, w, cin, 2 * d, ngf)
        new = lambda: torch.empty((b, h, w, d), dtype=torch.float32, device=self.device)
        rgba = torch.empty((b, d, h, w, 4), dtype=torch.float32, device=self.device) if want_f32 else None
        bw = new() if 'blend_weights' in extra_outputs else None
        al = new() if 'alpha' in extra_outputs else None
        ev = 0 if event_after_convs is None else event_after_convs.cuda_event
        if pfmt is None:
            N.check(N.lib.msi_net_plan_forward_rgba(plan.handle, packed.data_ptr(), net_input.data_ptr(), rgba.data_ptr(),
                                                    _ptr(bw), _ptr(al), 0, ws.data_ptr(), ws.numel(), self._stream(), ev),
                    "msi_net_plan_forward_rgba")
        else:
            codes = torch.empty((b, d, h, w, 4), dtype=torch.uint8 if pfmt == 'rgba8' else torch.float16, device=self.device)
            N.check(N.lib.msi_net_plan_forward_layers(plan.handle, packed.data_ptr(), net_input.data_ptr(), _ptr(rgba), codes.data_ptr(),
                                                      self.LAYER_FORMATS[pfmt], _ptr(bw), _ptr(al), 0, ws.data_ptr(), ws.numel(),
                                                      self._stream(), ev), "msi_net_plan_forward_layers")
        self._last_forward = (plan, ws)
        pred = {}
        if rgba is not None:
            pred['rgba_layers'] = rgba.permute(0, 2, 3, 1, 4)
        if pfmt is not None:
            pred['packed_layers'] = PackedLayers(codes, pfmt)
        if bw is not None:
            pred['blend_weights'] = bw
        if al is not None:
            pred['alphas'] = al
        if 'psv' in extra_outputs:
            pred['psv'] = net_input
        return pred

    def assemble_layers(self, net_input, msi_pred, num_msi_planes, extra_outputs='', which_color_pred='blend_psv'):
        """layer_prediction of infer_msi (msi.py:130-147, 177-188, 223-242, 258-268; outputs :276-289)."""
        b, h, w, _ = net_input.shape
        d = num_msi_planes
        color = self.COLOR_SCHEMES[which_color_pred]
        new = lambda: torch.empty((b, h, w, d), dtype=torch.float32, device=self.device)
        rgba = torch.empty((b, d, h, w, 4), dtype=torch.float32, device=self.device)
        # msi.py:280-285: blend_weights only for the 'blend' schemes, bg_blend_weights where they exist (blend_bg_psv)
        bw = new() if 'blend_weights' in extra_outputs and 'blend' in which_color_pred else None
        bgw = new() if bw is not None and which_color_pred == 'blend_bg_psv' else None
        al = new() if 'alpha' in extra_outputs else None
        N.check(N.lib.msi_assemble_rgba_color_f32(
            net_input.data_ptr(), 1 if net_input.dtype == torch.bfloat16 else 0, msi_pred.data_ptr(), color,
            rgba.data_ptr(), _ptr(bw), _ptr(al), _ptr(bgw), b, h, w, d, self._stream()), "msi_assemble_rgba_color_f32")
        pred = {'rgba_layers': rgba.permute(0, 2, 3, 1, 4)}
        if bw is not None:
            pred['blend_weights'] = bw
        if bgw is not None:
            pred['bg_blend_weights'] = bgw
        if al is not None:
            pred['alphas'] = al
        if 'psv' in extra_outputs:
            pred['psv'] = net_input
        return pred

    # ------------------------------------------------------------------ msi.py:384-452
    def _native_layers(self, rgba_layers):
        if isinstance(rgba_layers, MipLayers):
            raise TypeError("this method does not read mip-mapped stacks: render a MipLayers with render_views or render_ods_pair, or "
                            "pass its level 0, .base")
        if isinstance(rgba_layers, FactoredLayers):
            raise TypeError("this method reads layer stacks, not their factors: render a FactoredLayers with render_views or "
                            "render_ods_pair, or build its stack with materialize_layers first")
        if isinstance(rgba_layers, SparseLayers):
            raise TypeError("this method does not read sparse stacks: render a SparseLayers with render_views or render_ods_pair "
                            "(MSI; border='wrap') or with mpi_render_views / cube_render_views (border='edge'), or expand it with "
                            "densify_layers first")
        if isinstance(rgba_layers, PackedLayers):
            raise TypeError("this method reads fp32 layer stacks only: render a PackedLayers with render_views (MSI) or "
                            "mpi_render_views (MPI), or expand it with unpack_layers first")
        rgba_layers = rgba_layers.to(device=self.device, dtype=torch.float32) if torch.is_tensor(rgba_layers) \
            else self._f32(rgba_layers)
        if rgba_layers.dim() != 5 or rgba_layers.shape[-1] != 4:
            raise ValueError("rgba_layers must be [B,H,W,D,4]")
        native = rgba_layers.permute(0, 3, 1, 2, 4)   # [B,D,H,W,4]
        return native if native.is_contiguous() else native.contiguous()

    @staticmethod
    def _domain_guard(tgt_pos, pose, planes, swap_xz):
        """Host-side only (never a device sync): the ray origin -- tgt_pos with its axes permuted as the ray model does
        (spherical.py:286-288 / :390-392) and taken through the FULL 4x4 pose, translation included (spherical.py:303-310)
        -- must lie inside the innermost sphere, or intersect_sphere takes the square root of a negative number
        (spherical.py:316-318) and the int cast of the NaN pixel coordinate is undefined.  Skipped when either input
        lives on the device: render_kernel clamps a negative discriminant to zero (finite, not reference-defined) and ORs
        MSI_RENDER_STATUS_ORIGIN_OUTSIDE into the model's status word -- render_status() reports it."""
        if any(torch.is_tensor(t) and t.is_cuda for t in (tgt_pos, pose, planes)):
            return
        tp = np.asarray(torch.as_tensor(tgt_pos), dtype=np.float64).reshape(-1, 3)
        c = np.stack([tp[:, 2], tp[:, 1], tp[:, 0]] if swap_xz else [tp[:, 0], tp[:, 1], -tp[:, 2]], axis=1)
        ps = np.asarray(torch.as_tensor(pose), dtype=np.float64).reshape(-1, 4, 4)
        if ps.shape[0] == 1 and c.shape[0] > 1:
            ps = np.repeat(ps, c.shape[0], axis=0)
        if ps.shape[0] != c.shape[0]:
            return      # the batch check that follows reports it
        origin = np.einsum('bij,bj->bi', ps[:, :3, :3], c) + ps[:, :3, 3]
        pl = np.asarray(planes.cpu() if torch.is_tensor(planes) else planes, dtype=np.float64)
        if np.any(np.linalg.norm(origin, axis=1) >= np.abs(pl).min()):
            raise ValueError("the target ray origin (pose @ tgt_pos) must lie inside the innermost sphere (radius %g)"
                             % np.abs(pl).min())

    def _render_args(self, rgba_layers, tgt_pose_rt, tgt_pos, planes):
        native = self._native_layers(rgba_layers)
        b, d, h, w, _ = native.shape
        self._domain_guard(tgt_pos, tgt_pose_rt, planes, swap_xz=True)
        pose = self._f32(tgt_pose_rt).reshape(-1, 4, 4)
        # batch size is taken from tgt_pose_rt in the reference (msi.py:419); broadcast a single pose
        if pose.shape[0] == 1 and b > 1:
            pose = pose.expand(b, 4, 4).contiguous()
        pos = self._f32(tgt_pos).reshape(-1, 3)
        if pose.shape[0] != b or pos.shape[0] != b:
            raise ValueError("tgt_pose_rt / tgt_pos batch must match rgba_layers")
        depths = self._depths(planes, d)
        return native, pose, pos, depths, self._trig(h, w), (b, d, h, w)

    def msi_render_equirect_view(self, rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics):
        """Render a target view from an MSI representation -> [B,H,W,3] (msi.py:407-429)."""
        out, _ = self.msi_render_equirect_view_and_depth(rgba_layers, tgt_pose_rt, tgt_pos, planes,
                                                         intrinsics, want_rgb=True, want_depth=False)
        return out

    def msi_render_equirect_depth(self, rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics):
        """Composite the normalised layer index instead of colour (msi.py:384-405)."""
        _, out = self.msi_render_equirect_view_and_depth(rgba_layers, tgt_pose_rt, tgt_pos, planes,
                                                         intrinsics, want_rgb=False, want_depth=True)
        return out

    def msi_render_equirect_view_and_depth(self, rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics,
                                           want_rgb=True, want_depth=True):
        """Both outputs of test.py:149-159 from ONE warp (the reference recomputes it)."""
        native, pose, pos, depths, trig, (b, d, h, w) = self._render_args(rgba_layers, tgt_pose_rt, tgt_pos, planes)
        rgb = torch.empty((b, h, w, 3), dtype=torch.float32, device=self.device) if want_rgb else None
        dep = torch.empty((b, h, w, 3), dtype=torch.float32, device=self.device) if want_depth else None
        N.check(N.lib.msi_render_equirect_f32(native.data_ptr(), pose.data_ptr(), pos.data_ptr(),
                                              depths.data_ptr(), trig.data_ptr(), b, h, w, d,
                                              _ptr(rgb), _ptr(dep), self._render_status.data_ptr(), self._stream()),
                "msi_render_equirect_f32")
        return rgb, dep

    def msi_render_equirect_view_single(self, rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics):
        """Warped, un-composited layers [D,B,H,W,4] (msi.py:431-452)."""
        native, pose, pos, depths, trig, (b, d, h, w) = self._render_args(rgba_layers, tgt_pose_rt, tgt_pos, planes)
        out = torch.empty((d, b, h, w, 4), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_project_layers_f32(native.data_ptr(), pose.data_ptr(), pos.data_ptr(),
                                             depths.data_ptr(), trig.data_ptr(), b, h, w, d,
                                             out.data_ptr(), self._render_status.data_ptr(), self._stream()), "msi_project_layers_f32")
        return out

    def msi_render_equirect_depth_single(self, rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics):
        """msi.py:454-473: the same warped, un-composited layers as msi_render_equirect_view_single (the reference's
        two functions have identical bodies; the caller composites the index channel, test.py:374-382)."""
        return self.msi_render_equirect_view_single(rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics)

    # ------------------------------------------------------------------ msi.py:502-525
    def msi_render_ods_view(self, rgba_layers, order, jitter_pose, tgt_pos, planes, intrinsics):
        """Render the left (order=+1) / right (order=-1) ODS eye from an MSI -> [B,H,W,3].
        `tgt_pos` is accepted and unused, as in the reference (spherical.intersect_ods ignores it)."""
        native = self._native_layers(rgba_layers)
        b, d, h, w, _ = native.shape
        pose = self._f32(jitter_pose).reshape(-1, 4, 4)
        if pose.shape[0] == 1 and b > 1:
            pose = pose.expand(b, 4, 4).contiguous()
        intr = self._f32(intrinsics).reshape(-1, 3, 3)
        if pose.shape[0] != b or intr.shape[0] != b:
            raise ValueError("jitter_pose / intrinsics batch must match rgba_layers")
        depths = self._depths(planes, d)
        out = torch.empty((b, h, w, 3), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_render_ods_f32(native.data_ptr(), pose.data_ptr(), intr.data_ptr(), depths.data_ptr(),
                                         self._trig(h, w).data_ptr(), b, h, w, d, int(order), out.data_ptr(),
                                         self._render_status.data_ptr(), self._stream()), "msi_render_ods_f32")
        return out

    # ------------------------------------------------------------------ msi.py:475-500
    @staticmethod
    def _crop_pose(viewing_window):
        """projector.py:78-86: from_euler([0, vw*pi/2, 0]) = Ry, zero translation; fp32 entries are
        the correctly rounded cos/sin of the fp32 angle."""
        ang = float(np.float32(viewing_window * np.pi / 2.0))
        c, s = np.float32(np.cos(ang)), np.float32(np.sin(ang))
        m = np.eye(4, dtype=np.float32)
        m[0, 0] = c; m[0, 2] = s; m[2, 0] = -s; m[2, 2] = c
        return m

    def msi_render_perspective_view(self, rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics,
                                    viewing_window=3, psp_height=270, psp_width=480):
        """Perspective crop of the MSI -> [B,psp_height,psp_width,3].  As in the reference, the
        passed tgt_pose_rt only supplies the batch size: the crop rotation replaces it
        (projector.py:78-86)."""
        native = self._native_layers(rgba_layers)
        b, d, h, w, _ = native.shape
        crop = np.tile(self._crop_pose(viewing_window)[None], (b, 1, 1))
        self._domain_guard(tgt_pos, crop, planes, swap_xz=False)
        pose = self._f32(crop)
        pos = self._f32(tgt_pos).reshape(-1, 3)
        if pos.shape[0] != b:
            raise ValueError("tgt_pos batch must match rgba_layers")
        depths = self._depths(planes, d)
        out = torch.empty((b, psp_height, psp_width, 3), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_render_perspective_f32(native.data_ptr(), pose.data_ptr(), pos.data_ptr(), depths.data_ptr(),
                                                 b, h, w, d, psp_height, psp_width, out.data_ptr(),
                                                 self._render_status.data_ptr(), self._stream()),
                "msi_render_perspective_f32")
        return out

    # ------------------------------------------------------------------ viewer: many views of one MSI per launch
    # ('ods' is not a camera code of the native library: it has its own entry point, msi_render_ods_views)
    CAMERAS = {'equirect': N.MSI_CAMERA_EQUIRECT, 'pinhole': N.MSI_CAMERA_PINHOLE, 'ods': None}

    def _view_stack(self, rgba_layers, planes, who, border):
        """What a viewer's launch takes from its stack -- a stack [B,H,W,D,4], a PackedLayers or a SparseLayers made with the keep
        rule `border` -> (the entry point's leading arguments: (pool, table, layer_start, format) or (layers, format); the suffix
        of its name: '_sparse', '_packed' or '_f32'; (b, d, h, w); planes; the stack on this device, which the caller holds until
        the launch).  planes=None takes the planes a PackedLayers or SparseLayers carries.  A sparse stack made for the other kind
        of surface is refused: an edge-rule stack misses tiles a sphere render reads across the border, and a sphere stack in a
        planar viewer is almost always a mistake.
        A FactoredLayers (render_views alone): the leading arguments are msi_hres_layers' inputs and sizes, the suffix is '_factored'.
        A MipLayers (render_views alone): (layers, format, mips, levels), the suffix is '_mip'."""
        if isinstance(rgba_layers, MipLayers):
            if who != "render_views":
                raise TypeError("%s does not read mip-mapped stacks: pass the MipLayers' level 0, .base" % who)
            mip = rgba_layers if rgba_layers.data.device == self.device else rgba_layers.to(self.device)
            planes = mip.planes if planes is None else planes
            if planes is None:
                raise ValueError("%s: planes is required (this MipLayers carries none)" % who)
            fmt = N.MSI_LAYERS_F32 if mip.format == 'f32' else self.LAYER_FORMATS[mip.format]
            return (mip.data.data_ptr(), fmt, mip.mips.data_ptr(), mip.levels), "_mip", tuple(mip.data.shape[:4]), planes, mip
        if isinstance(rgba_layers, FactoredLayers):
            if who != "render_views":
                raise TypeError("%s reads layer stacks, not their factors: build the stack of a FactoredLayers with "
                                "materialize_layers first" % who)
            f = rgba_layers if rgba_layers.device == self.device else rgba_layers.to(self.device)
            planes = f.planes if planes is None else planes
            head, keep = self._hres_head(f, planes)
            return head, "_factored", self._factored_dims(f), planes, keep
        if isinstance(rgba_layers, SparseLayers):
            if rgba_layers.border != border:
                raise TypeError("%s reads SparseLayers made with border=%r, not %r: expand this one with densify_layers and "
                                "sparsify_layers(..., border=%r) the result" % (who, border, rgba_layers.border, border))
            sparse = rgba_layers if rgba_layers.pool.device == self.device else rgba_layers.to(self.device)
            planes = sparse.planes if planes is None else planes
            if planes is None:
                raise ValueError("%s: planes is required (this SparseLayers carries none)" % who)
            b, h, w, d = sparse.shape
            lead = (sparse.pool.data_ptr(), sparse.table.data_ptr(), sparse.layer_start.data_ptr(), self.LAYER_FORMATS[sparse.format])
            return lead, "_sparse", (b, d, h, w), planes, sparse
        packed = rgba_layers if isinstance(rgba_layers, PackedLayers) else None
        if packed is not None:
            native = packed.data if packed.data.device == self.device else packed.data.to(self.device)
            if planes is None:
                planes = packed.planes
        else:
            native = self._native_layers(rgba_layers)
        if planes is None:
            raise ValueError("%s: planes is required (only a PackedLayers that carries its planes may leave it out)" % who)
        fmt = self.LAYER_FORMATS[packed.format] if packed is not None else N.MSI_LAYERS_F32
        return (native.data_ptr(), fmt), "_packed" if packed is not None else "_f32", tuple(native.shape[:4]), planes, native

    def _view_poses(self, name, tgt_pose, tgt_pos, b):
        """Per-view poses [B,V,4,4] and, where the camera has them, positions [B,V,3] ([V,4,4] / [V,3] when B = 1) -> fp32
        (pose, pos, V)."""
        pose = self._f32(tgt_pose)
        pos = None if tgt_pos is None else self._f32(tgt_pos)
        if b == 1 and pose.dim() == 3 and (pos is None or pos.dim() == 2):
            pose, pos = pose[None], None if pos is None else pos[None]
        if pose.dim() != 4 or pose.shape[0] != b or tuple(pose.shape[2:]) != (4, 4):
            raise ValueError("%s must be [B,V,4,4] with B = %d (or [V,4,4] for B = 1), got %s" % (name, b, tuple(pose.shape)))
        v = pose.shape[1]
        if pos is not None and tuple(pos.shape) != (b, v, 3):
            raise ValueError("tgt_pos must be [B,V,3] = %s, got %s" % ((b, v, 3), tuple(pos.shape)))
        return pose, pos, v

    def _pinhole_intrinsics(self, intrinsics, b, v):
        """[B,V,3,3] or one [3,3] for every view -> fp32 [B*V,3,3]."""
        intr = self._f32(intrinsics).reshape(-1, 3, 3)
        if intr.shape[0] == 1:
            intr = intr.expand(b * v, 3, 3).contiguous()
        if intr.shape[0] != b * v:
            raise ValueError("intrinsics must be [B,V,3,3] or [3,3]")
        return intr

    def _view_outputs(self, b, v, oh, ow, want_rgb, want_depth):
        rgb = torch.empty((b, v, oh, ow, 3), dtype=torch.float32, device=self.device) if want_rgb else None
        dep = torch.empty((b, v, oh, ow), dtype=torch.float32, device=self.device) if want_depth else None
        return rgb, dep

    def render_views(self, rgba_layers, tgt_pose_rt, tgt_pos, planes=None, camera='equirect', intrinsics=None, size=None,
                     want_rgb=True, want_depth=True, eye=None, baseline=None, lod_bias=0.0, max_anisotropy=1.0):
        """V views of each MSI in ONE launch (msi_render_views_f32; no reference counterpart) -> (rgb, depth):
        rgb [B,V,h,w,3] in [-1,1], depth [B,V,h,w] (one channel: msi_render_equirect_depth(...)[..., 0]); either is None
        when switched off.

        rgba_layers [B,H,W,D,4] (a permuted view of the native [B,D,H,W,4] stack goes through without a copy);
        tgt_pose_rt [B,V,4,4], tgt_pos [B,V,3] ([V,4,4] / [V,3] when B = 1).  Each view has the meaning of the pair of
        msi_render_equirect_view: the ray direction is rotated by pose[:3,:3], the ray origin is
        pose @ (tgt_pos[2], tgt_pos[1], tgt_pos[0], 1), and view v of sample b samples stack b only.
        size = (h, w), shared by every view: default (H, W) for 'equirect', required for 'pinhole'.
          'equirect': pixel (i, j) takes its ray from the lat-long grid of the OUTPUT size (at (H, W) each view is
                      bit-identical to msi_render_equirect_view_and_depth with its pose).
          'pinhole':  intrinsics [B,V,3,3] or one [3,3] for every view, in pixels (fx, fy, cx, cy); pixel (i, j) looks
                      along (1, (i + 0.5 - cy) / fy, (j + 0.5 - cx) / fx) before the pose: forward +x, image-down +y,
                      image-right +z -- with an identity pose the centre pixel looks where the centre of an equirect
                      render looks, with the same orientation.
          'ods':      the eye panoramas of a stereo 360 frame (msi_render_ods_views): the equirect camera with the ray origin
                      moved onto the viewing circle around the head position, (tgt_pos[2] + sin S * e, tgt_pos[1],
                      tgt_pos[0] - cos S * e) before the pose, e = eye * baseline.  eye (required): +1 / 'left' (the
                      reference's order = +1, the ref image) or -1 / 'right' (the src image), one for every view or an array
                      [V] / [B,V].  baseline: a float, [B] or [B,V] (>= 0); None takes intrinsics[:, 0, 0], where the reference
                      keeps it (intrinsics [B,3,3] or [1,3,3]).  With baseline 0 it is the equirect camera, bit for bit; the
                      image is upright, i.e. msi_render_ods_view's flipped left-to-right.  eye and baseline belong to this
                      camera only.
        Host-side poses and positions are checked for every view before the launch (ValueError when an origin is not
        inside the innermost sphere -- for 'ods': when |pose @ swap(tgt_pos)| + |e| >= min |planes|, which keeps the whole
        circle inside); device-side ones are flagged through render_status().
        rgba_layers may be a PackedLayers (pack_layers; msi_render_views_packed): the kernel gathers from the compact stack
        itself and the outputs are bit-identical to rendering unpack_layers(rgba_layers).  planes=None then takes the planes
        the PackedLayers carries (ValueError when it carries none); for an fp32 stack planes is required.
        rgba_layers may be a SparseLayers (sparsify_layers; msi_render_views_sparse), for all three cameras: every output element
        compares == to the render of the PackedLayers it was made from and of densify_layers(rgba_layers) -- the same bits, except
        that a zero may differ in sign -- provided colours are finite where alpha is zero (always so for rgba8).  planes=None
        takes the planes it carries.  Only a stack made with border='wrap' (the default) is accepted: TypeError otherwise.
        rgba_layers may be a FactoredLayers (hres_factors; msi_render_views_factored), for all three cameras: no stack exists, every
        tap evaluates the texel hres_layers would have stored, and every output element compares == to the render of
        materialize_layers(rgba_layers)['rgba_layers'] (a zero may differ in sign; image values finite).  planes=None takes the
        planes it carries.
        rgba_layers may be a MipLayers (build_mips; msi_render_views_mip), for all three cameras: every layer's texel is blended from
        the two pyramid levels that bracket the pixel's footprint on that layer (trilinear filtering; the rule is in msi_hip.h), so
        a view SMALLER than the stack -- a thumbnail, a wide field of view, the poles, the far side of a translated viewpoint --
        does not alias.  lod_bias is added to the level of detail: > 0 blurs, < 0 sharpens, <= -64 is the plain render of .base bit
        for bit (so is a pixel whose footprint is at most one texel on every layer, and a MipLayers of one level).  With
        max_anisotropy = 1 (the default) the filter is isotropic: near the stack's poles, where a footprint is many texels long and
        one wide, it blurs along latitude too.  max_anisotropy = A in (1, 16] (msi_render_views_aniso) takes the level from the
        footprint's minor axis and up to 2 ceil((A - 1) / 2) + 1 trilinear samples along its major axis (the rule is in msi_hip.h):
        the ceiling and the floor of a tilted, rolled or translated view stay sharp without aliasing; away from the poles it is the
        trilinear render.  It costs time where footprints are long and is opt-in.  planes=None takes the planes it carries.
        lod_bias and max_anisotropy belong to a MipLayers: anything but 0 / 1 with another kind of stack is a ValueError."""
        if camera not in self.CAMERAS:
            raise ValueError("camera must be 'equirect', 'pinhole' or 'ods', not %r" % (camera,))
        if camera != 'ods' and (eye is not None or baseline is not None):
            raise ValueError("render_views: eye and baseline belong to camera='ods', not %r" % (camera,))
        if camera == 'ods' and eye is None:
            raise ValueError("render_views: camera='ods' needs eye (+1 / 'left' or -1 / 'right', or an array [V] / [B,V])")
        if not (want_rgb or want_depth):
            raise ValueError("render_views: want_rgb and want_depth are both False")
        lod_bias = float(lod_bias)
        if lod_bias != lod_bias:
            raise ValueError("render_views: lod_bias is NaN")
        if lod_bias != 0.0 and not isinstance(rgba_layers, MipLayers):
            raise ValueError("render_views: lod_bias belongs to a MipLayers (build_mips), this stack has one level")
        max_anisotropy = float(max_anisotropy)
        if not 1.0 <= max_anisotropy <= N.MSI_ANISO_MAX:                   # (a NaN fails the comparison)
            raise ValueError("render_views: max_anisotropy must be in [1, %d], not %r" % (N.MSI_ANISO_MAX, max_anisotropy))
        if max_anisotropy != 1.0 and not isinstance(rgba_layers, MipLayers):
            raise ValueError("render_views: max_anisotropy belongs to a MipLayers (build_mips), this stack is filtered isotropically")
        lead, suffix, (b, d, h, w), planes, _keep = self._view_stack(rgba_layers, planes, "render_views", 'wrap')   # (_keep: alive until the launch)
        if camera != 'ods':
            self._domain_guard(tgt_pos, tgt_pose_rt, planes, swap_xz=True)
        pose, pos, v = self._view_poses("tgt_pose_rt", tgt_pose_rt, tgt_pos, b)
        depths = self._depths(planes, d)
        intr = trig = radius = None
        if camera == 'pinhole':
            if size is None or intrinsics is None:
                raise ValueError("camera='pinhole' needs size=(h, w) and intrinsics")
            oh, ow = int(size[0]), int(size[1])
            intr = self._pinhole_intrinsics(intrinsics, b, v)
        else:
            oh, ow = (h, w) if size is None else (int(size[0]), int(size[1]))
            if camera == 'ods':
                radius = self._eye_radius(eye, baseline, intrinsics, b, v)
                self._ods_domain_guard(tgt_pos, tgt_pose_rt, planes, radius)
                radius = self._f32(radius).reshape(b * v)
            trig = self._trig(oh, ow)
        rgb, dep = self._view_outputs(b, v, oh, ow, want_rgb, want_depth)
        # four entry points, one argument list: they differ in the stack, the camera's tables and whether there is a camera code ('ods' has none;
        # from a sparse stack it is the equirect code with an eye_radius table)
        views = (pose.data_ptr(), pos.data_ptr())
        shape, code = (b, v, h, w, d), (self.CAMERAS[camera],)
        out = (oh, ow, _ptr(rgb), _ptr(dep), self._render_status.data_ptr(), self._stream())
        name = "msi_render_views" + suffix
        if suffix == "_sparse":
            args = lead + views + (_ptr(intr), _ptr(radius), depths.data_ptr(), _ptr(trig)) + shape \
                + ((N.MSI_CAMERA_EQUIRECT,) if camera == 'ods' else code)
        elif suffix == "_mip":                    # (msi_render_views_sparse's list behind the stack and lod_bias; max_anisotropy > 1: the anisotropic twin)
            if max_anisotropy != 1.0:
                name = "msi_render_views_aniso"
            args = lead + ((lod_bias,) if max_anisotropy == 1.0 else (lod_bias, max_anisotropy)) + views + (_ptr(intr), _ptr(radius), depths.data_ptr(), _ptr(trig)) + shape \
                + ((N.MSI_CAMERA_EQUIRECT,) if camera == 'ods' else code)
        elif suffix == "_factored":               # (depths and the stack's sizes are in `lead`: msi_hres_layers' argument list)
            args = lead + views + (_ptr(intr), _ptr(radius), _ptr(trig), v) + ((N.MSI_CAMERA_EQUIRECT,) if camera == 'ods' else code)
        elif camera == 'ods':
            name = "msi_render_ods_views"
            args = lead + views + (radius.data_ptr(), depths.data_ptr(), trig.data_ptr()) + shape
        else:                                     # (msi_render_views_f32 takes no format code)
            args = lead[:1 if suffix == "_f32" else 2] + views + (_ptr(intr), depths.data_ptr(), _ptr(trig)) + shape + code
        N.check(getattr(N.lib, name)(*(args + out)), name)
        return rgb, dep

    EYES = {'left': 1.0, 'right': -1.0}

    def _eye_radius(self, eye, baseline, intrinsics, b, v):
        """The signed radius e = eye * baseline of every view, [B,V]: a numpy array when eye and baseline are host-side (values
        checked here: eye in +-1, baseline finite and >= 0), a device tensor when either lives on the device (shapes only: no sync)."""
        if isinstance(eye, str):
            if eye not in self.EYES:
                raise ValueError("eye must be +1 / 'left' or -1 / 'right', not %r" % (eye,))
            eye = self.EYES[eye]
        if baseline is None:
            if intrinsics is None:
                raise ValueError("camera='ods' needs baseline, or intrinsics [B,3,3] that carry it in [:, 0, 0]")
            intr = intrinsics if torch.is_tensor(intrinsics) else np.asarray(intrinsics, dtype=np.float32)
            if tuple(intr.shape) not in ((b, 3, 3), (1, 3, 3)):
                raise ValueError("intrinsics must be [B,3,3] = %s or [1,3,3], got %s" % ((b, 3, 3), tuple(intr.shape)))
            baseline = intr[:, 0, 0] if intr.shape[0] == b else intr[0, 0, 0]
        if any(torch.is_tensor(t) and t.is_cuda for t in (eye, baseline)):
            ey, bl = self._f32(eye), self._f32(baseline)
            broadcast = torch.broadcast_to
        else:
            ey = np.asarray(eye.cpu() if torch.is_tensor(eye) else eye, dtype=np.float32)
            bl = np.asarray(baseline.cpu() if torch.is_tensor(baseline) else baseline, dtype=np.float32)
            broadcast = lambda x, shape: np.array(np.broadcast_to(x, shape), dtype=np.float32)      # (a writable copy)
            if not np.all(np.abs(ey) == 1.0):
                raise ValueError("eye must be +1 (left) or -1 (right)")
            if not (np.all(np.isfinite(bl)) and np.all(bl >= 0)):
                raise ValueError("baseline must be finite and >= 0")
        if tuple(ey.shape) not in ((), (v,), (b, v)):
            raise ValueError("eye must be a scalar, [V] or [B,V] = %s, got %s" % ((b, v), tuple(ey.shape)))
        if tuple(bl.shape) not in ((), (b,), (b, v)):
            raise ValueError("baseline must be a scalar, [B] or [B,V] = %s, got %s" % ((b, v), tuple(bl.shape)))
        if bl.ndim == 1:
            bl = bl.reshape(b, 1)                                   # ([B]: per sample, also when B = V)
        return broadcast(ey * bl, (b, v))

    @staticmethod
    def _ods_domain_guard(tgt_pos, pose, planes, radius):
        """_domain_guard for the ODS camera (host-side only, skipped when any input lives on the device: the kernel flags those):
        every point of the viewing circle is within |e| of the head position pose @ swap(tgt_pos), so
        |pose @ swap(tgt_pos)| + |e| < min |planes| is sufficient for every origin of the view to lie inside the innermost sphere."""
        if any(torch.is_tensor(t) and t.is_cuda for t in (tgt_pos, pose, planes, radius)):
            return
        tp = np.asarray(torch.as_tensor(tgt_pos), dtype=np.float64).reshape(-1, 3)
        c = np.stack([tp[:, 2], tp[:, 1], tp[:, 0]], axis=1)
        ps = np.asarray(torch.as_tensor(pose), dtype=np.float64).reshape(-1, 4, 4)
        e = np.abs(np.asarray(radius, dtype=np.float64).reshape(-1))
        if ps.shape[0] != c.shape[0] or e.shape[0] != c.shape[0]:
            return      # the shape checks report it
        centre = np.einsum('bij,bj->bi', ps[:, :3, :3], c) + ps[:, :3, 3]
        pl = np.asarray(planes.cpu() if torch.is_tensor(planes) else planes, dtype=np.float64)
        if not np.all(np.linalg.norm(centre, axis=1) + e < np.abs(pl).min()):
            raise ValueError("the ODS viewing circle (|pose @ tgt_pos| + |eye * baseline|) must lie inside the innermost sphere "
                             "(radius %g)" % np.abs(pl).min())

    PAIR_LAYOUTS = ('views', 'top_bottom')

    def _ods_pair_views(self, who, b, tgt_pose_rt, tgt_pos, baseline, layout):
        """What render_ods_pair and cube_render_ods_pair share: one pose [B,4,4] (or [4,4]; default identity) and head position
        [B,3] (or [3]; default 0) per sample -> the two views' (pose [B,2,4,4], pos [B,2,3], eye = left then right), with layout and
        the baseline's shape (a float or [B]) checked."""
        if layout not in self.PAIR_LAYOUTS:
            raise ValueError("layout must be 'views' or 'top_bottom', not %r" % (layout,))

        def per_view(x, default, tail):
            if x is None:
                return np.tile(default, (b, 2) + (1,) * len(tail))
            x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float32))
            if tuple(x.shape) == tail:
                x = x.expand((b,) + tail)
            if tuple(x.shape) != (b,) + tail:
                raise ValueError("%s: expected %s or %s, got %s" % (who, (b,) + tail, tail, tuple(x.shape)))
            return x[:, None].expand((b, 2) + tail)
        pose = per_view(tgt_pose_rt, np.eye(4, dtype=np.float32), (4, 4))
        pos = per_view(tgt_pos, np.zeros(3, np.float32), (3,))
        if baseline is not None:
            shape = tuple(baseline.shape) if hasattr(baseline, "shape") else np.shape(baseline)
            if shape not in ((), (b,)):
                raise ValueError("%s: baseline must be a float or [B] = %s, got %s" % (who, (b,), shape))
        return pose, pos, np.array([1.0, -1.0], np.float32)

    @staticmethod
    def _pair_layout(rgb, dep, layout, want_rgb, want_depth):
        """[B,2,h,w,...] as the caller asked for it: 'top_bottom' is the SAME storage as [B,2h,w,...] (a view, no copy)."""
        if layout == 'top_bottom':
            rgb = rgb.view(rgb.shape[0], 2 * rgb.shape[2], rgb.shape[3], 3) if rgb is not None else None
            dep = dep.view(dep.shape[0], 2 * dep.shape[2], dep.shape[3]) if dep is not None else None
        return (rgb, dep) if want_rgb and want_depth else rgb if want_rgb else dep

    def render_ods_pair(self, rgba_layers, planes=None, baseline=None, intrinsics=None, tgt_pose_rt=None, tgt_pos=None, size=None,
                        layout='views', want_depth=False, lod_bias=0.0, max_anisotropy=1.0):
        """Both eyes of each sample's stereo 360 frame in ONE launch (render_views(camera='ods') with V = 2: left then right,
        sharing one pose and head position) -> rgb, or (rgb, depth) with want_depth.
        tgt_pose_rt [B,4,4] (or one [4,4]; default identity), tgt_pos [B,3] (or one [3]; default 0); planes, baseline,
        intrinsics and size as in render_views -- with the sample's own baseline, identity pose and position 0 the two views are
        the input pair (ref image = left) as the MSI reproduces it.
        layout='views': rgb [B,2,h,w,3], depth [B,2,h,w].  'top_bottom': the SAME storage as [B,2h,w,3] / [B,2h,w], left eye on
        top -- the delivery format of 360 players, without a copy.  lod_bias and max_anisotropy: render_views', for a MipLayers."""
        b = (rgba_layers.data if isinstance(rgba_layers, PackedLayers) else rgba_layers).shape[0]     # (SparseLayers / FactoredLayers / MipLayers.shape: (B, H, W, D))
        pose, pos, eye = self._ods_pair_views("render_ods_pair", b, tgt_pose_rt, tgt_pos, baseline, layout)
        rgb, dep = self.render_views(rgba_layers, pose, pos, planes, camera='ods', intrinsics=intrinsics, size=size,
                                     want_rgb=True, want_depth=want_depth, eye=eye, baseline=baseline, lod_bias=lod_bias,
                                     max_anisotropy=max_anisotropy)
        return self._pair_layout(rgb, dep, layout, True, want_depth)

    # ------------------------------------------------------------------ compact stacks (matryodshka_amd/packed.py)
    LAYER_FORMATS = {'rgba8': N.MSI_LAYERS_RGBA8, 'rgba16f': N.MSI_LAYERS_RGBA16F}

    def build_mips(self, layers, levels=None, planes=None):
        """A stack -> MipLayers (matryodshka_amd/mips.py): the stack as level 0 plus the levels 1 .. L-1 of its pyramid in one buffer,
        about a third of the stack's bytes, one launch that reads the stack once (msi_build_mips; the rule is in msi_hip.h and, in
        numpy, mips.build_mips_np).  `layers` is an fp32 stack [B,H,W,D,4] (a permuted view of the native stack goes through without a
        copy) or a PackedLayers, whose format the levels keep.  levels: L in 1..6 with H and W multiples of 2^(L-1) and a top level of
        at least 2 x 2 (ValueError); None takes the largest L the sizes allow.  `planes`, or else the planes a PackedLayers carries,
        travel with the result, which goes into render_views / render_ods_pair."""
        if isinstance(layers, (MipLayers, SparseLayers, FactoredLayers)):
            raise TypeError("build_mips takes an fp32 stack or a PackedLayers, not a %s%s" % (
                type(layers).__name__, ": pass its level 0, .base" if isinstance(layers, MipLayers) else ""))
        if isinstance(layers, PackedLayers):
            data = layers.data if layers.data.device == self.device else layers.data.to(self.device)
            planes = layers.planes if planes is None else planes
            base, fmt = PackedLayers(data, layers.format, planes), self.LAYER_FORMATS[layers.format]
        else:
            base = data = self._native_layers(layers)
            fmt = N.MSI_LAYERS_F32
        b, d, h, w, _ = data.shape
        if planes is not None and len(planes) != d:
            raise ValueError("len(planes) != number of layers")
        levels = max_mip_levels(h, w) if levels is None else check_mip_levels(h, w, levels)
        mips = torch.empty((sum(int(np.prod(s)) for s in mip_level_shapes(data.shape, levels)),), dtype=data.dtype, device=self.device)
        N.check(N.lib.msi_build_mips(data.data_ptr(), fmt, b, d, h, w, levels, mips.data_ptr(), self._stream()), "msi_build_mips")
        return MipLayers(base, mips, levels, planes)

    def pack_layers(self, rgba_layers, format='rgba8', planes=None):
        """fp32 stack [B,H,W,D,4] -> PackedLayers in `format` ('rgba8': 4 bytes per texel, 'rgba16f': 8; the rule is in
        packed.py / msi_hip.h), one streaming kernel (msi_pack_layers).  A permuted view of the native [B,D,H,W,4] stack goes
        through without a copy, as in render_views.  `planes`, when given, travel with the stack."""
        if format not in PACKED_FORMATS:
            raise ValueError("format must be one of %s, not %r" % (PACKED_FORMATS, format))
        native = self._native_layers(rgba_layers)
        b, d, h, w, _ = native.shape
        if planes is not None and len(planes) != d:
            raise ValueError("len(planes) != number of layers")
        data = torch.empty((b, d, h, w, 4), dtype=torch.uint8 if format == 'rgba8' else torch.float16, device=self.device)
        N.check(N.lib.msi_pack_layers(native.data_ptr(), self.LAYER_FORMATS[format], data.data_ptr(), b * d * h * w, self._stream()),
                "msi_pack_layers")
        return PackedLayers(data, format, planes)

    def sparsify_layers(self, layers, format='rgba8', planes=None, border='wrap'):
        """A stack -> SparseLayers (matryodshka_amd/sparse.py: only the 4 x 16 tiles a render can see are stored).  border='wrap': the
        tiles a sphere render can see (render_views, render_ods_pair; msi_sparse_index_tiles); border='edge': those a render that
        never reads the opposite border can see -- mpi_render_views on a [B,H,W,D,4] MPI and cube_render_views on [6B,S,S,D,4] cube
        faces (msi_sparse_index_tiles_edge).  `layers` is
        an fp32 stack [B,H,W,D,4], packed first with pack_layers(layers, format), or a PackedLayers, whose own format is kept.
        H % 4 == 0 and W % 16 == 0 are required (ValueError).  `planes`, or else the planes a PackedLayers carries, travel with the stack.
        Three launches (msi_sparse_index_tiles: two, msi_sparse_gather_tiles) around one host synchronisation: the pool's size is
        data-dependent.  The result is the same bytes every time and equals sparse.sparsify_np of the codes."""
        if isinstance(layers, SparseLayers):
            raise TypeError("sparsify_layers takes an fp32 stack or a PackedLayers, not a SparseLayers")
        if isinstance(layers, MipLayers):
            raise TypeError("sparsify_layers takes an fp32 stack or a PackedLayers, not a MipLayers: pass its level 0, .base")
        if isinstance(layers, FactoredLayers):
            raise TypeError("sparsify_layers takes an fp32 stack or a PackedLayers, not a FactoredLayers: build its sparse stack with "
                            "materialize_layers(..., sparse=True)")
        if border not in BORDERS:
            raise ValueError("border must be one of %s, not %r" % (BORDERS, border))
        pk = layers if isinstance(layers, PackedLayers) else self.pack_layers(layers, format, planes)
        planes = pk.planes if planes is None else planes
        data = pk.data if pk.data.device == self.device else pk.data.to(self.device)
        b, d, h, w, _ = data.shape
        if planes is not None and len(planes) != d:
            raise ValueError("len(planes) != number of layers")
        if h % TILE_H or w % TILE_W:
            raise ValueError("a sparse stack needs H %% %d == 0 and W %% %d == 0, not %d x %d" % (TILE_H, TILE_W, h, w))
        fmt = self.LAYER_FORMATS[pk.format]
        table = torch.empty((b, d, h // TILE_H, w // TILE_W), dtype=torch.int32, device=self.device)
        counts = torch.empty((b * d,), dtype=torch.int32, device=self.device)
        index = "msi_sparse_index_tiles" if border == 'wrap' else "msi_sparse_index_tiles_edge"
        N.check(getattr(N.lib, index)(data.data_ptr(), fmt, b, d, h, w, table.data_ptr(), counts.data_ptr(), self._stream()), index)
        layer_start = torch.zeros((b * d + 1,), dtype=torch.int64, device=self.device)
        if b * d:
            layer_start[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(layer_start[-1].item())
        pool = torch.empty((total, TILE_H, TILE_W, 4), dtype=data.dtype, device=self.device)
        if total:
            N.check(N.lib.msi_sparse_gather_tiles(data.data_ptr(), fmt, table.data_ptr(), layer_start.data_ptr(), b, d, h, w,
                                                  pool.data_ptr(), self._stream()), "msi_sparse_gather_tiles")
        return SparseLayers(table, layer_start, pool, pk.format, planes, border=border)

    def densify_layers(self, sparse):
        """SparseLayers (of either keep rule) -> the PackedLayers it stands for, all-zero bytes in dropped tiles (msi_sparse_expand)."""
        if not isinstance(sparse, SparseLayers):
            raise TypeError("densify_layers takes a SparseLayers")
        sparse = sparse if sparse.pool.device == self.device else sparse.to(self.device)
        b, h, w, d = sparse.shape
        data = torch.empty((b, d, h, w, 4), dtype=sparse.pool.dtype, device=self.device)
        if data.numel():
            N.check(N.lib.msi_sparse_expand(sparse.pool.data_ptr(), sparse.table.data_ptr(), sparse.layer_start.data_ptr(),
                                            self.LAYER_FORMATS[sparse.format], b, d, h, w, data.data_ptr(), self._stream()),
                    "msi_sparse_expand")
        return PackedLayers(data, sparse.format, sparse.planes)

    def unpack_layers(self, packed):
        """PackedLayers -> fp32 [B,H,W,D,4], a permuted view of a new native [B,D,H,W,4] stack (msi_unpack_layers)."""
        if not isinstance(packed, PackedLayers):
            raise TypeError("unpack_layers takes a PackedLayers" + (
                " (expand a SparseLayers with densify_layers first)" if isinstance(packed, SparseLayers) else
                " (build the fp32 stack of a FactoredLayers with materialize_layers)" if isinstance(packed, FactoredLayers) else
                " (pass a MipLayers' level 0, .base)" if isinstance(packed, MipLayers) else ""))
        data = packed.data if packed.data.device == self.device else packed.data.to(self.device)
        b, d, h, w, _ = data.shape
        native = torch.empty((b, d, h, w, 4), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_unpack_layers(data.data_ptr(), self.LAYER_FORMATS[packed.format], native.data_ptr(), b * d * h * w,
                                        self._stream()), "msi_unpack_layers")
        return native.permute(0, 2, 3, 1, 4)

    # ------------------------------------------------------------------ test.py:283-394
    def _hres_inputs(self, who, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes, intrinsics,
                     ref_pose_inv, sweep='ODS'):
        """What the high-res builders hand to their launches, checked: (bw, al, hres_ref, hres_src, cur, intr, depths, trig).  sweep='ODS'
        (hres_layers, hres_layers_sparse): the model's own sweep, ODS models only; sweep='PP' (their mpi_ twins): the method names the
        sweep, any model, trig is None and intr is [B,3,3]."""
        if sweep == 'ODS' and self.input_type != 'ODS':
            raise ValueError("%s sweeps the sphere (input_type='ODS' models); the perspective sweep is mpi_%s" % (who, who))
        bw, al = self._f32(blend_weights), self._f32(alphas)
        if bw.dim() != 4 or bw.shape != al.shape:
            raise ValueError("%s: blend_weights and alphas must be [B,H,W,D] and agree" % who)
        b, h, w, d = bw.shape
        depths = self._depths(planes, d)
        hres_ref = self.preprocess_image(raw_hres_ref_image)
        hres_src = self.preprocess_image(raw_hres_src_image)
        if hres_ref.shape[0] != b or hres_ref.shape[3] != 3 or hres_src.shape != hres_ref.shape:
            raise ValueError("%s: images must be [B,Hh,Wh,3], agree, and have the batch of blend_weights" % who)
        cur = self._current_poses(ref_pose, src_pose, ref_pose_inv, b)
        intr = self._f32(intrinsics)
        if sweep == 'ODS':
            return bw, al, hres_ref, hres_src, cur, intr, depths, self._trig(hres_ref.shape[1], hres_ref.shape[2])
        if intr.numel() != b * 9:
            raise ValueError("%s: intrinsics (of the high-res images) must be [B,3,3] with B = %d" % (who, b))
        if hres_ref.shape[1] < 2 or hres_ref.shape[2] < 2:
            raise ValueError("%s: a perspective sweep needs images of at least 2 x 2" % who)
        return bw, al, hres_ref, hres_src, cur, intr, depths, None

    def hres_layers(self, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                    intrinsics, ref_pose_inv=None, layer_format='f32'):
        """The high-res layer stack of test.py:283-394 in ONE launch (msi_hres_layers): the high-res ODS sweep of both images,
        the align_corners bilinear resize of the low-res blend_weights / alphas ([B,H,W,D], in (0,1): infer_msi's
        extra_outputs) and the blend, without the [B,Hh,Wh,6D] sweep volume or the upsampled tensor in memory.
        layer_format as in infer_layers: 'f32' in the request -> result['rgba_layers'] ([B,Hh,Wh,D,4], a permuted view of the
        native stack); 'rgba8' / 'rgba16f' -> result['packed_layers'], a PackedLayers that carries `planes` and goes straight
        into render_views; ('f32', packed) writes both in the same launch.  The fp32 stack has the bits of format_network_input
        -> msi_resize_bilinear_f32 -> msi_assemble_rgba_scaled_f32, the packed one those of pack_layers of it; a packed-only
        request allocates nothing but the packed stack.  ODS models only (fp32 or bf16: the high-res colours are fp32 either
        way).  Poses as in format_network_input (ref_pose_inv computed on the host when absent).  hres_layers_sparse builds the
        packed stack sparse, without the dense one."""
        formats = self._layer_formats(layer_format)
        return self._hres_build("hres_layers", 'ODS', blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                                intrinsics, ref_pose_inv, *formats)

    def hres_layers_sparse(self, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                           intrinsics, ref_pose_inv=None, layer_format='rgba8'):
        """hres_layers' packed stack as a SparseLayers, without the dense stack: the arguments of hres_layers, layer_format 'rgba8'
        or 'rgba16f' alone (fp32 pools are not built), Hh % 4 == 0 and Wh % 16 == 0 (else ValueError) -> {'sparse_layers':
        SparseLayers} that carries `planes`: the table, layer_start and pool that sparsify_layers(hres_layers(...)['packed_layers'])
        has for the same request, bit for bit; it goes straight into render_views / render_ods_pair, save and densify_layers.
        A texel's alpha is the resized low-res alpha, whatever the images hold, so msi_hres_index_tiles decides the kept tiles
        from `alphas` alone; after the one host synchronisation sparsify_layers has too (the pool's size is data-dependent)
        msi_hres_layers_sparse computes the texels of kept tiles only, straight into the pool.  Only table, counts, layer_start
        and pool are allocated.  ODS models only."""
        formats = self._layer_formats(layer_format)
        return self._hres_build_sparse("hres_layers_sparse", 'ODS', blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose,
                                       planes, intrinsics, ref_pose_inv, *formats)

    def hres_factors(self, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes, intrinsics,
                     ref_pose_inv=None):
        """The arguments of hres_layers -> the FactoredLayers (matryodshka_amd/factored.py) of the stack hres_layers would build: its
        checks, its preprocessing of the two images and its pose composition, and no launch beyond those.  The result goes straight
        into render_views / render_ods_pair (msi_render_views_factored: the stack is never allocated) and into save; every other
        method wants materialize_layers of it.  ODS models only."""
        if self.input_type != 'ODS':
            raise ValueError("hres_factors sweeps the sphere (input_type='ODS' models); the perspective sweep has no factored stack")
        bw, al, hres_ref, hres_src, cur, intr, _depths, _trig = self._hres_inputs(
            "hres_factors", blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes, intrinsics, ref_pose_inv)
        return FactoredLayers(bw, al, hres_ref, hres_src, cur[0], cur[1], intr, planes)

    @staticmethod
    def _factored_dims(f):
        """(B, D, Hh, Wh) of the stack a FactoredLayers stands for."""
        b, hh, hw, d = f.shape
        return (b, d, hh, hw)

    def _hres_head(self, f, planes):
        """msi_hres_layers' inputs and sizes from a FactoredLayers on this device -> (the argument tuple, the tensors behind its pointers: `f`,
        the planes on the device -- a NEW tensor when `planes` is a tensor that had to be moved or converted -- and the trig table; the
        caller holds them until the launch)."""
        b, d, hh, hw = self._factored_dims(f)
        h, w = f.alphas.shape[1], f.alphas.shape[2]
        depths, trig = self._depths(planes, d), self._trig(hh, hw)
        head = (f.ref_image.data_ptr(), f.src_image.data_ptr(), f.ref_pose.data_ptr(), f.src_pose.data_ptr(), f.intrinsics.data_ptr(),
                depths.data_ptr(), trig.data_ptr(), f.blend_weights.data_ptr(), f.alphas.data_ptr(), b, h, w, hh, hw, d)
        return head, (f, depths, trig)

    def materialize_layers(self, factors, layer_format='f32', sparse=False):
        """FactoredLayers -> the stack it stands for: what hres_layers returns for the same request (msi_hres_layers on the stored
        pieces: result['rgba_layers'] and / or result['packed_layers'], layer_format as there), or with sparse=True what
        hres_layers_sparse returns ({'sparse_layers': ...}; layer_format 'rgba8' or 'rgba16f')."""
        if not isinstance(factors, FactoredLayers):
            raise TypeError("materialize_layers takes a FactoredLayers (hres_factors)")
        f = factors if factors.device == self.device else factors.to(self.device)
        want_f32, pfmt = self._layer_formats(layer_format)
        (head, _keep), shape = self._hres_head(f, f.planes), self._factored_dims(f)     # (_keep: alive until the launch)
        if not sparse:
            return self._hres_dense("msi_hres_layers", head, shape, f.planes, want_f32, pfmt)
        if want_f32 or pfmt is None:
            raise ValueError("materialize_layers(sparse=True) takes layer_format 'rgba8' or 'rgba16f' alone (fp32 pools are not built)")
        return self._hres_sparse("msi_hres_index_tiles", "msi_hres_layers_sparse", head, f.alphas, tuple(f.alphas.shape[1:3]), shape, f.planes,
                                 pfmt, 'wrap')

    def mpi_hres_layers(self, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                        intrinsics, ref_pose_inv=None, layer_format='f32'):
        """hres_layers for perspective images, in ONE launch (msi_pp_hres_layers): the high-res perspective plane sweep of both
        images (ref = foreground, src = background), the align_corners resize of the low-res blend_weights / alphas [B,H,W,D]
        and the blend -> what hres_layers returns (result['rgba_layers'] [B,Hh,Wh,D,4] and / or result['packed_layers'], which
        carries `planes`), for mpi_render_views and, with six faces per sample, cube_render_views.  `intrinsics` [B,3,3] are
        those of the HIGH-RES images.  The fp32 stack has the bits of two msi_perspective_plane_sweep_f32 ->
        msi_resize_bilinear_f32 -> msi_assemble_rgba_scaled_f32, the packed one those of pack_layers of it; the [B,Hh,Wh,6D]
        volume and the upsampled tensor never exist, and a packed-only request allocates nothing but the packed stack.  Works on
        any model, like mpi_render_views: the method names the sweep.  mpi_hres_layers_sparse builds the packed stack sparse."""
        formats = self._layer_formats(layer_format)
        return self._hres_build("mpi_hres_layers", 'PP', blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                                intrinsics, ref_pose_inv, *formats)

    def mpi_hres_layers_sparse(self, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                               intrinsics, ref_pose_inv=None, layer_format='rgba8'):
        """mpi_hres_layers' packed stack as a SparseLayers with border='edge', without the dense stack: layer_format 'rgba8' or
        'rgba16f' alone, Hh % 4 == 0 and Wh % 16 == 0 (else ValueError) -> {'sparse_layers': SparseLayers} that carries `planes`:
        the table, layer_start and pool of sparsify_layers(mpi_hres_layers(...)['packed_layers'], border='edge'), bit for bit; it
        goes straight into mpi_render_views / cube_render_views.  msi_hres_index_tiles_edge decides the kept tiles from `alphas`
        alone (a texel's alpha is the resized alpha), msi_pp_hres_layers_sparse computes the texels of kept tiles only.  Only
        table, counts, layer_start and pool are allocated.  Any model."""
        formats = self._layer_formats(layer_format)
        return self._hres_build_sparse("mpi_hres_layers_sparse", 'PP', blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose,
                                       src_pose, planes, intrinsics, ref_pose_inv, *formats)

    def _hres_build(self, who, sweep, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes, intrinsics,
                    ref_pose_inv, want_f32, pfmt):
        """hres_layers (sweep='ODS': msi_hres_layers) and mpi_hres_layers (sweep='PP': msi_pp_hres_layers, the same parameters without trig);
        (want_f32, pfmt) = _layer_formats of the caller's request."""
        bw, al, hres_ref, hres_src, cur, intr, depths, trig = self._hres_inputs(
            who, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes, intrinsics, ref_pose_inv, sweep)
        b, h, w, d = bw.shape
        hh, hw = hres_ref.shape[1], hres_ref.shape[2]
        name = "msi_hres_layers" if sweep == 'ODS' else "msi_pp_hres_layers"
        trig_arg = (trig.data_ptr(),) if sweep == 'ODS' else ()
        return self._hres_dense(name, (hres_ref.data_ptr(), hres_src.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(), intr.data_ptr(),
                                       depths.data_ptr(), *trig_arg, bw.data_ptr(), al.data_ptr(), b, h, w, hh, hw, d), (b, d, hh, hw), planes,
                                want_f32, pfmt)

    def _hres_dense(self, name, head, shape, planes, want_f32, pfmt):
        """The dense high-res builders' outputs and launch: entry point `name` called with `head` (its inputs and sizes), the fp32 and / or packed
        stack of `shape` = (B, D, H, W) allocated for it, and the result wrapped as hres_layers documents."""
        rgba = torch.empty(shape + (4,), dtype=torch.float32, device=self.device) if want_f32 else None
        codes = None
        if pfmt is not None:
            codes = torch.empty(shape + (4,), dtype=torch.uint8 if pfmt == 'rgba8' else torch.float16, device=self.device)
        N.check(getattr(N.lib, name)(*head, _ptr(rgba), _ptr(codes), self.LAYER_FORMATS.get(pfmt, N.MSI_LAYERS_F32), self._stream()), name)
        out = {}
        if rgba is not None:
            out['rgba_layers'] = rgba.permute(0, 2, 3, 1, 4)
        if codes is not None:
            out['packed_layers'] = PackedLayers(codes, pfmt, planes)
        return out

    def _hres_sparse(self, index, fill, head, alphas, low, shape, planes, pfmt, border):
        """The sparse high-res builders: the table of `shape` = (B, D, H, W) from the low-res alphas ([B,h,w,D], low = (h, w)) by entry point `index`,
        layer_start by cumsum, the pool (one host synchronisation: its size is data-dependent), and entry point `fill` called with `head` (its
        inputs and sizes) for the texels of kept tiles -> {'sparse_layers': SparseLayers}."""
        b, d, hh, hw = shape
        if hh % TILE_H or hw % TILE_W:
            raise ValueError("a sparse stack needs H %% %d == 0 and W %% %d == 0, not %d x %d" % (TILE_H, TILE_W, hh, hw))
        fmt = self.LAYER_FORMATS[pfmt]
        table = torch.empty((b, d, hh // TILE_H, hw // TILE_W), dtype=torch.int32, device=self.device)
        counts = torch.empty((b * d,), dtype=torch.int32, device=self.device)
        N.check(getattr(N.lib, index)(alphas.data_ptr(), fmt, b, low[0], low[1], hh, hw, d, table.data_ptr(), counts.data_ptr(), self._stream()), index)
        layer_start = torch.zeros((b * d + 1,), dtype=torch.int64, device=self.device)
        if b * d:
            layer_start[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(layer_start[-1].item())
        pool = torch.empty((total, TILE_H, TILE_W, 4), dtype=torch.uint8 if pfmt == 'rgba8' else torch.float16, device=self.device)
        if total:
            N.check(getattr(N.lib, fill)(*head, table.data_ptr(), layer_start.data_ptr(), pool.data_ptr(), fmt, self._stream()), fill)
        return {'sparse_layers': SparseLayers(table, layer_start, pool, pfmt, planes, border=border)}

    def _hres_build_sparse(self, who, sweep, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes,
                           intrinsics, ref_pose_inv, want_f32, pfmt):
        """hres_layers_sparse (sweep='ODS': msi_hres_index_tiles, msi_hres_layers_sparse, border 'wrap') and mpi_hres_layers_sparse
        (sweep='PP': msi_hres_index_tiles_edge, msi_pp_hres_layers_sparse, border 'edge'); (want_f32, pfmt) = _layer_formats of the
        caller's request."""
        if want_f32 or pfmt is None:
            raise ValueError("%s takes layer_format 'rgba8' or 'rgba16f' alone (fp32 pools are not built)" % who)
        bw, al, hres_ref, hres_src, cur, intr, depths, trig = self._hres_inputs(
            who, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose, planes, intrinsics, ref_pose_inv, sweep)
        b, h, w, d = bw.shape
        hh, hw = hres_ref.shape[1], hres_ref.shape[2]
        index, fill, border = (("msi_hres_index_tiles", "msi_hres_layers_sparse", 'wrap') if sweep == 'ODS' else
                               ("msi_hres_index_tiles_edge", "msi_pp_hres_layers_sparse", 'edge'))
        trig_arg = (trig.data_ptr(),) if sweep == 'ODS' else ()
        head = (hres_ref.data_ptr(), hres_src.data_ptr(), cur[0].data_ptr(), cur[1].data_ptr(), intr.data_ptr(), depths.data_ptr(), *trig_arg,
                bw.data_ptr(), al.data_ptr(), b, h, w, hh, hw, d)
        return self._hres_sparse(index, fill, head, al, (h, w), (b, d, hh, hw), planes, pfmt, border)

    def msi_render_equirect_hres(self, blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image,
                                 ref_pose, src_pose, tgt_pose_rt, tgt_pos, planes, intrinsics,
                                 ref_pose_inv=None):
        """High-res re-render of test.py:283-394 as two launches: the reference loops over the planes
        on the host (one sess.run + numpy composite per plane, to fit its GPU memory); here hres_layers
        builds the whole fp32 high-res stack in one kernel (no sweep volume in memory) and one render
        composites it (on an input_type='PP' model: mpi_hres_layers, the perspective sweep).  To keep the stack, or to get it
        packed, call hres_layers / mpi_hres_layers itself.
        blend_weights / alphas: the low-res [B,H,W,D] outputs of infer_msi(extra_outputs=
        'blend_weights alphas') (test.py:264-271 saves them as .npy).  Returns (rgb, depth), both
        [B,Hh,Wh,3] float (rgb in [-1,1], depth = composited plane index / D as test.py:374-382)."""
        if self.input_type == 'ODS':
            rgba_layers = self.hres_layers(blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose,
                                           planes, intrinsics, ref_pose_inv=ref_pose_inv, layer_format='f32')['rgba_layers']
            return self.msi_render_equirect_view_and_depth(rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics)
        # perspective inputs: the same two launches through the PP builder (the bits of the sweep, resize and assembly it replaced here)
        rgba_layers = self.mpi_hres_layers(blend_weights, alphas, raw_hres_ref_image, raw_hres_src_image, ref_pose, src_pose,
                                           planes, intrinsics, ref_pose_inv=ref_pose_inv, layer_format='f32')['rgba_layers']
        return self.msi_render_equirect_view_and_depth(rgba_layers, tgt_pose_rt, tgt_pos, planes, intrinsics)

    # ------------------------------------------------------------------ msi.py:527-548
    def mpi_render_view(self, rgba_layers, tgt_pose, planes, intrinsics, intrinsics_inv=None):
        """Render a target perspective view from plane layers by per-plane inverse homographies
        (zero-padding bilinear) -> [B,H,W,3].  `intrinsics_inv` replaces the hidden graph input
        `intrinsics_inv:0` (homography.py:52); default inverse(intrinsics)."""
        native = self._native_layers(rgba_layers)
        b, d, h, w, _ = native.shape
        pose = self._f32(tgt_pose).reshape(-1, 4, 4)
        intr = self._f32(intrinsics).reshape(-1, 3, 3)
        if intrinsics_inv is None:
            intrinsics_inv = torch.linalg.inv(intr.cpu().double()).float()
        intr_inv = self._f32(intrinsics_inv).reshape(-1, 3, 3)
        if pose.shape[0] != b or intr.shape[0] != b or intr_inv.shape[0] != b:
            raise ValueError("tgt_pose / intrinsics batch must match rgba_layers")
        depths = self._depths(planes, d)
        out = torch.empty((b, h, w, 3), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_mpi_render_f32(native.data_ptr(), pose.data_ptr(), intr.data_ptr(), intr_inv.data_ptr(),
                                         depths.data_ptr(), b, h, w, d, out.data_ptr(), self._stream()),
                "msi_mpi_render_f32")
        return out

    def _view_intrinsics(self, k, b, v, what):
        """[B,V,3,3], [B,3,3] or [3,3] -> fp32 [B*V,3,3] (one camera per view), on the device it came from."""
        k = k.float() if torch.is_tensor(k) else torch.as_tensor(np.asarray(k, dtype=np.float32))
        if k.dim() == 2:
            k = k[None, None]
        elif k.dim() == 3:
            k = k[:, None]
        if k.dim() != 4 or tuple(k.shape[2:]) != (3, 3) or k.shape[0] not in (1, b) or k.shape[1] not in (1, v):
            raise ValueError("%s must be [B,V,3,3], [B,3,3] or [3,3] with B = %d, V = %d, got %s" % (what, b, v, tuple(k.shape)))
        return k.expand(b, v, 3, 3).reshape(b * v, 3, 3)

    def mpi_render_views(self, rgba_layers, tgt_pose, planes=None, intrinsics=None, tgt_intrinsics=None, intrinsics_inv=None,
                         size=None, want_rgb=True, want_depth=True):
        """V views of each MPI in ONE launch (msi_mpi_render_views; no reference counterpart) -> (rgb, depth): rgb
        [B,V,h,w,3] in [-1,1], depth [B,V,h,w] (the composited plane index / D of over_composite_depth, one channel); either
        is None when switched off.  Works on any model (ODS or PP, f32 or bf16): the stack is what matters.

        rgba_layers [B,H,W,D,4] (a permuted view of the native [B,D,H,W,4] stack goes through without a copy) or a
        PackedLayers, which the kernel gathers from directly: the outputs are bit-identical to rendering
        unpack_layers(rgba_layers).  planes=None takes the planes a PackedLayers carries (ValueError when it carries none);
        for an fp32 stack planes is required.
        tgt_pose [B,V,4,4] ([V,4,4] when B = 1): each has the meaning of mpi_render_view's tgt_pose, and view v of sample b
        samples stack b only.  intrinsics: the stack's camera, [B,3,3] or [3,3].  The target camera is EITHER
        tgt_intrinsics ([B,V,3,3], [B,3,3] or [3,3]; inverted on the host in fp64 and rounded to fp32, as mpi_render_view
        does) OR intrinsics_inv (same shapes, used as given); neither means inverse(intrinsics), both is a ValueError.
        size = (h, w), shared by every view, default (H, W); the target camera is in pixels of that size.  At size (H, W)
        with the same intrinsics_inv, rgb[:, v] is bit-identical to mpi_render_view with tgt_pose[:, v].
        rgba_layers may be a SparseLayers made with border='edge' (sparsify_layers; msi_mpi_render_views_sparse): every output
        element compares == to the render of the PackedLayers it was made from (a zero may differ in sign), provided colours
        are finite where alpha is zero; planes=None takes the planes it carries.  A border='wrap' stack is refused (TypeError)."""
        if not (want_rgb or want_depth):
            raise ValueError("mpi_render_views: want_rgb and want_depth are both False")
        if tgt_intrinsics is not None and intrinsics_inv is not None:
            raise ValueError("mpi_render_views: pass tgt_intrinsics or intrinsics_inv, not both")
        if intrinsics is None:
            raise ValueError("mpi_render_views: intrinsics (the stack's camera) is required")
        lead, suffix, (b, d, h, w), planes, _keep = self._view_stack(rgba_layers, planes, "mpi_render_views", 'edge')
        pose, _, v = self._view_poses("tgt_pose", tgt_pose, None, b)
        pose = pose.contiguous()
        intr = self._f32(intrinsics).reshape(-1, 3, 3)
        if intr.shape[0] == 1 and b > 1:
            intr = intr.expand(b, 3, 3)
        if intr.shape[0] != b:
            raise ValueError("intrinsics must be [B,3,3] with B = %d or [3,3], got %s" % (b, tuple(intr.shape)))
        intr = intr.contiguous()
        if intrinsics_inv is not None:
            k_inv = self._view_intrinsics(intrinsics_inv, b, v, "intrinsics_inv")
        else:
            k_t = self._view_intrinsics(intrinsics if tgt_intrinsics is None else tgt_intrinsics, b, v, "tgt_intrinsics")
            k_inv = torch.linalg.inv(k_t.cpu().double()).float()
        k_inv = self._f32(k_inv.contiguous())
        depths = self._depths(planes, d)
        oh, ow = (h, w) if size is None else (int(size[0]), int(size[1]))
        rgb, dep = self._view_outputs(b, v, oh, ow, want_rgb, want_depth)
        tail = (pose.data_ptr(), intr.data_ptr(), k_inv.data_ptr(), depths.data_ptr(), b, v, h, w, d, oh, ow, _ptr(rgb), _ptr(dep),
                self._stream())
        name = "msi_mpi_render_views" + (suffix if suffix == "_sparse" else "")
        N.check(getattr(N.lib, name)(*(lead + tail)), name)
        return rgb, dep

    # ------------------------------------------------------------------ cube-map viewer of the PP path (cubemap.py has the conventions)
    def equirect_to_cube(self, image, face_size, intrinsics=None):
        """Panorama [B,H,W,C] (fp32, C in 1..4) -> its six face images [B,6,S,S,C] (msi_equirect_to_cube_f32; no reference
        counterpart), faces in cubemap.FACE_ROTATIONS order.  Texel (ix, iy) of face f looks along R_f K^-1 (ix, iy, 1);
        intrinsics = the face camera K, [3,3] or [B,3,3], default cubemap.default_face_intrinsics(S).  Bilinear on the
        panorama's lat-long grid, wrapping in longitude and clamping in latitude.  The panorama is taken as a
        single-centre (equirectangular) image: the faces of an ODS panorama are not perspective images."""
        from . import cubemap
        image = self._f32(image)
        if image.dim() != 4 or not 1 <= image.shape[-1] <= 4:
            raise ValueError("equirect_to_cube: image must be [B,H,W,C] with C in 1..4, got %s" % (tuple(image.shape),))
        b, h, w, c = image.shape
        s = int(face_size)
        if s < 1:
            raise ValueError("equirect_to_cube: face_size must be positive")
        k = self._f32(cubemap.default_face_intrinsics(s) if intrinsics is None else intrinsics).reshape(-1, 3, 3)
        if k.shape[0] == 1 and b > 1:
            k = k.expand(b, 3, 3)
        if k.shape[0] != b:
            raise ValueError("equirect_to_cube: intrinsics must be [3,3] or [B,3,3] with B = %d" % b)
        k = k.contiguous()
        out = torch.empty((b, 6, s, s, c), dtype=torch.float32, device=self.device)
        N.check(N.lib.msi_equirect_to_cube_f32(image.data_ptr(), k.data_ptr(), b, h, w, c, s, out.data_ptr(), self._stream()),
                "msi_equirect_to_cube_f32")
        return out

    CUBE_FILTERINGS = ('clamp', 'seamless')

    def cube_render_views(self, rgba_layers, tgt_pose_rt, tgt_pos, planes=None, stack_intrinsics=None, camera='equirect',
                          intrinsics=None, size=None, want_rgb=True, want_depth=True, filtering='clamp', eye=None, baseline=None):
        """V views of each CUBE of six face stacks in ONE launch (msi_cube_render_views; no reference counterpart) ->
        (rgb [B,V,h,w,3] in [-1,1], depth [B,V,h,w]: the composited plane index / D of over_composite_depth); either is None
        when switched off.  The planar twin of render_views; works on any model (the stack is what matters).

        rgba_layers [6B,S,S,D,4] (a permuted view of the native [6B,D,S,S,4] stack -- what infer_cube / the PP network writes
        for 6B faces -- goes through without a copy) or a PackedLayers of it; face f of sample b is entry 6 b + f, faces in
        cubemap.FACE_ROTATIONS order.  Layer d of the six faces forms a cube shell of half-side planes[d]; a ray from inside
        the innermost shell meets each shell once, on one face, and the D shells are composited far to near.  planes=None
        takes the planes a PackedLayers carries (ValueError when it carries none); an fp32 stack needs planes.
        stack_intrinsics: the camera K shared by a sample's six faces, [3,3] or [B,3,3], integer-pixel convention of the MPI
        path; default cubemap.default_face_intrinsics(S).  With that default (fx = cx = S/2) a face covers [-1, 1 - 2/S] in
        tan space, not [-1, 1]: the renderer CLAMPS TO THE EDGE inside the chosen face -- it neither zero-pads nor fetches
        from the neighbouring face.  Pass fx = cx = (S-1)/2 for symmetric faces.
        tgt_pose_rt [B,V,4,4], tgt_pos [B,V,3] ([V,4,4] / [V,3] when B = 1), camera, intrinsics: render_views' cameras and
        pose model, unchanged; its frame (forward +x, down +y, right +z) maps to the cube frame (face 0's camera frame) by
        swapping x and z, so the centre of an equirect output looks at the centre of face 0 and one set of arguments renders
        an MSI and a cube stack of one scene.  size = (h, w) is required for every camera.
        Host-side poses and positions are checked before the launch (ValueError when an origin is not strictly inside the
        innermost shell: max |o_k| >= min planes); device-side ones are flagged through render_status().
        rgba_layers may be a SparseLayers of the faces made with border='edge' (sparsify_layers of the [6B,S,S,D,4] stack;
        msi_cube_render_views_sparse; whole tiles make S % 16 == 0, sparsify_layers refuses other sizes): every output element compares == to the render of the
        PackedLayers it was made from (a zero may differ in sign), provided colours are finite where alpha is zero, and the
        status word is the same; planes=None takes the planes it carries.  A border='wrap' stack is refused (TypeError).
        filtering='clamp' (default) is the rule above.  filtering='seamless' (msi_cube_render_views_seamless; dense stacks, the
        default stack_intrinsics only) filters ACROSS the cube's edges: with fx = cx = S/2 a face stores nothing on its +x / +y
        edge, so clamping repeats the last texel over a one-texel band along every cube edge, while the neighbouring face
        usually stores exactly the missing sample (its column 0 or row 0).  u, v are clamped to [0, S]; a tap at x = S or y = S
        is a virtual texel: the texel of the first other face (ascending index) that stores that cube point, else the mean of
        the clamped texels of the faces meeting there (cubemap.virtual_texel is the host statement of the rule, the cubemap
        module's comment the full text).  8 of the 12 cube edges are stored by one face (continuous filter), 2 by none
        (right/down, back/down: the mean, continuous over two texels), 2 by both (up/back, up/left: each face keeps its own
        texel, so a step in the CONTENT of the two faces stays -- in-range texels are never overridden).  Away from the strip
        (u, v <= S-1) the pixels are the clamp render's, bit for bit; a packed render keeps the bits of the render of the
        unpacked stack.  A host-side stack_intrinsics other than the default raises ValueError; one given on the device is not
        read back: such a sample is rendered with the clamp rule and render_status() returns RENDER_STATUS_NOT_CUBE_CAMERA
        (2).  A SparseLayers raises TypeError (densify_layers it first): the edge keep rule guarantees four zero alphas only
        for footprints inside one face.
        camera='ods' (msi_cube_render_ods_views / _sparse): the eye panoramas of a stereo 360 frame, render_views' ODS camera on a
        cube -- the equirect camera with the ray origin on the viewing circle around the head position, (tgt_pos[2] + sin S * e,
        tgt_pos[1], tgt_pos[0] - cos S * e) before the pose, e = eye * baseline.  eye (required): +1 / 'left' or -1 / 'right', one
        for every view or an array [V] / [B,V]; baseline (REQUIRED here: a cube stack carries no ODS intrinsics to default from): a
        float, [B] or [B,V], >= 0.  Both belong to this camera only.  With baseline 0 it is the equirect camera, bit for bit.
        Works with filtering='seamless' and with a border='edge' SparseLayers (not both).  Host-side inputs must keep the whole
        circle strictly inside the innermost shell -- max_k |o_k| + |e| < min planes, o the posed head position (ValueError;
        cubemap.check_ods_circle_inside) --; device-side ones set RENDER_STATUS_ORIGIN_OUTSIDE when ANY pixel's origin is outside."""
        from . import cubemap
        ods = cubemap.check_ods_arguments(camera, eye, baseline)
        if filtering not in self.CUBE_FILTERINGS:
            raise ValueError("cube_render_views: filtering must be one of %s, not %r" % (self.CUBE_FILTERINGS, filtering))
        if not (want_rgb or want_depth):
            raise ValueError("cube_render_views: want_rgb and want_depth are both False")
        lead, suffix, native_shape, planes, _keep = self._view_stack(rgba_layers, planes, "cube_render_views", 'edge')
        if filtering == 'seamless' and suffix == "_sparse":
            raise TypeError("cube_render_views: filtering='seamless' takes dense stacks only (a cross-edge footprint is outside the "
                            "edge keep rule of a SparseLayers); expand it with densify_layers first")
        shape = lambda t: tuple(t.shape) if hasattr(t, "shape") else tuple(np.asarray(t).shape)
        b, v, s, d, oh, ow = cubemap.cube_view_shapes(native_shape + (4,), shape(tgt_pose_rt), shape(tgt_pos), size)
        radius = self._eye_radius(eye, baseline, None, b, v) if ods else None      # ([B,V]: host values are checked there)
        if not any(torch.is_tensor(t) and t.is_cuda for t in (tgt_pos, tgt_pose_rt, planes, radius)):
            host = [np.asarray(torch.as_tensor(t)) for t in (tgt_pos, tgt_pose_rt, planes)]
            if ods:
                cubemap.check_ods_circle_inside(*(host + [radius]))
            else:
                cubemap.check_origin_inside(*host)
        pose, pos = self._f32(tgt_pose_rt).reshape(b * v, 4, 4), self._f32(tgt_pos).reshape(b * v, 3)
        depths = self._depths(planes, d)
        if filtering == 'seamless' and stack_intrinsics is not None and not (torch.is_tensor(stack_intrinsics) and stack_intrinsics.is_cuda):
            if not cubemap.is_default_face_intrinsics(np.asarray(torch.as_tensor(stack_intrinsics), dtype=np.float64), s):
                raise ValueError("cube_render_views: filtering='seamless' is defined for the cube camera fx = fy = cx = cy = S/2 "
                                 "(cubemap.default_face_intrinsics) only")
        ks = self._f32(cubemap.default_face_intrinsics(s) if stack_intrinsics is None else stack_intrinsics).reshape(-1, 3, 3)
        if ks.shape[0] == 1 and b > 1:
            ks = ks.expand(b, 3, 3)
        if ks.shape[0] != b:
            raise ValueError("stack_intrinsics must be [3,3] or [B,3,3] with B = %d" % b)
        ks = ks.contiguous()
        intr, trig = None, None
        if camera == 'pinhole':
            if intrinsics is None:
                raise ValueError("camera='pinhole' needs intrinsics")
            intr = self._pinhole_intrinsics(intrinsics, b, v)
        else:
            trig = self._trig(oh, ow)
        rgb, dep = self._view_outputs(b, v, oh, ow, want_rgb, want_depth)
        out = (oh, ow, _ptr(rgb), _ptr(dep), self._render_status.data_ptr(), self._stream())
        if ods:            # (an entry point of its own, like msi_render_ods_views: eye_radius where the pinhole table goes, a filtering code, no camera code)
            radius = self._f32(radius).reshape(b * v)
            name = "msi_cube_render_ods_views" + (suffix if suffix == "_sparse" else "")
            tail = (pose.data_ptr(), pos.data_ptr(), radius.data_ptr(), ks.data_ptr(), depths.data_ptr(), trig.data_ptr(), b, v, s, d) \
                + (() if suffix == "_sparse" else (self.CUBE_FILTERINGS.index(filtering),))
        else:
            name = "msi_cube_render_views" + ("_seamless" if filtering == 'seamless' else suffix if suffix == "_sparse" else "")
            tail = (pose.data_ptr(), pos.data_ptr(), _ptr(intr), ks.data_ptr(), depths.data_ptr(), _ptr(trig), b, v, s, d, self.CAMERAS[camera])
        N.check(getattr(N.lib, name)(*(lead + tail + out)), name)
        return rgb, dep

    def cube_render_ods_pair(self, rgba_layers, planes=None, baseline=None, stack_intrinsics=None, tgt_pose_rt=None, tgt_pos=None,
                             size=None, layout='views', filtering='clamp', want_rgb=True, want_depth=False):
        """render_ods_pair for a cube: both eyes of each sample's stereo 360 frame in ONE launch (cube_render_views(camera='ods') with
        V = 2: left then right, sharing one pose and head position) -> rgb, depth, or (rgb, depth) when both are wanted.
        rgba_layers, planes, stack_intrinsics, size (required) and filtering as in cube_render_views; baseline (required) a float
        or [B]; tgt_pose_rt [B,4,4] (or one [4,4]; default identity), tgt_pos [B,3] (or one [3]; default 0).
        layout='views': rgb [B,2,h,w,3], depth [B,2,h,w].  'top_bottom': the SAME storage as [B,2h,w,3] / [B,2h,w], left eye on top
        -- the delivery format of 360 players, without a copy."""
        if isinstance(rgba_layers, MipLayers):
            raise TypeError("cube_render_ods_pair does not read mip-mapped stacks: pass the MipLayers' level 0, .base")
        shape = rgba_layers.data.shape if isinstance(rgba_layers, PackedLayers) else rgba_layers.shape
        if shape[0] == 0 or shape[0] % 6:
            raise ValueError("cube_render_ods_pair: the leading dimension is 6 faces per sample, %d is not a multiple of 6" % shape[0])
        b = shape[0] // 6
        pose, pos, eye = self._ods_pair_views("cube_render_ods_pair", b, tgt_pose_rt, tgt_pos, baseline, layout)
        rgb, dep = self.cube_render_views(rgba_layers, pose, pos, planes, stack_intrinsics=stack_intrinsics, camera='ods', size=size,
                                          want_rgb=want_rgb, want_depth=want_depth, filtering=filtering, eye=eye, baseline=baseline)
        return self._pair_layout(rgb, dep, layout, want_rgb, want_depth)

    SRC_SAMPLINGS = ('face', 'panorama')

    def _src_sampling(self, who, src_sampling):
        if src_sampling not in self.SRC_SAMPLINGS:
            raise ValueError("%s: src_sampling must be one of %s, not %r" % (who, self.SRC_SAMPLINGS, src_sampling))
        return src_sampling == 'panorama'

    def _cube_sweep_inputs(self, who, ref_faces, src_panorama, face_src_poses, face_intrinsics):
        """The checked fp32 inputs the panorama-sampling entry points share -> (ref_faces, panorama, eye, face_src, kf, B, S)."""
        ref_faces, pano = self._f32(ref_faces), self._f32(src_panorama)
        if ref_faces.dim() != 4 or ref_faces.shape[3] != 3 or ref_faces.shape[1] != ref_faces.shape[2] or ref_faces.shape[0] % 6:
            raise ValueError("%s: ref_faces must be [6B,S,S,3], got %s" % (who, tuple(ref_faces.shape)))
        b, s = ref_faces.shape[0] // 6, ref_faces.shape[1]
        if pano.dim() != 4 or pano.shape[0] != b or pano.shape[3] != 3 or pano.shape[1] < 2 or pano.shape[2] < 2:
            raise ValueError("%s: src_panorama must be [B,Hp,Wp,3] with B = %d and Hp, Wp >= 2, got %s" % (who, b, tuple(pano.shape)))
        if s < 2:
            raise ValueError("%s: a perspective sweep needs faces of at least 2 x 2" % who)
        face_src, kf = self._f32(face_src_poses), self._f32(face_intrinsics)
        if face_src.numel() != 6 * b * 16 or kf.numel() != 6 * b * 9:
            raise ValueError("%s: face_src_poses must be [6B,4,4] and face_intrinsics [6B,3,3] with 6B = %d" % (who, 6 * b))
        eye = torch.eye(4, dtype=torch.float32, device=self.device).expand(6 * b, 4, 4).contiguous()
        return ref_faces, pano, eye, face_src, kf, b, s

    def format_cube_input(self, ref_faces, src_panorama, face_src_poses, planes, face_intrinsics, dtype=None):
        """format_network_input for a cube whose source half is sampled from the source PANORAMA: ref_faces [6B,S,S,3] and
        src_panorama [B,Hp,Wp,3] (both preprocessed, [-1,1]), face_src_poses [6B,4,4] (cubemap.face_poses of the source pose),
        face_intrinsics [6B,3,3] -> net_input [6B,S,S,6D].  The ref half is the perspective sweep of the ref faces with the
        identity pose, as format_network_input computes it; in the src half a plane point of face f is looked up in the
        panorama along its own direction (include/msi_hip.h states the sample position), so a point that projects past the
        face's border gets the neighbouring face's content, not the opposite side of its own face.  The model's dtype decides
        as in format_network_input (dtype='f32' forces fp32): bf16 is one launch (msi_cube_sweep_volume_bf16), fp32 is
        msi_perspective_plane_sweep_f32 for the ref half and msi_cube_plane_sweep_f32 for the src half."""
        ref_faces, pano, eye, face_src, kf, b, s = self._cube_sweep_inputs("format_cube_input", ref_faces, src_panorama, face_src_poses,
                                                                          face_intrinsics)
        depths = self._planes(planes)
        nd = depths.numel()
        hp, wp = pano.shape[1], pano.shape[2]
        bf16 = (dtype or self.dtype) == 'bf16'
        psv = torch.empty((6 * b, s, s, 6 * nd), dtype=torch.bfloat16 if bf16 else torch.float32, device=self.device)
        if bf16:
            N.check(N.lib.msi_cube_sweep_volume_bf16(ref_faces.data_ptr(), pano.data_ptr(), eye.data_ptr(), face_src.data_ptr(), kf.data_ptr(),
                                                     depths.data_ptr(), b, hp, wp, s, nd, psv.data_ptr(), self._stream()),
                    "msi_cube_sweep_volume_bf16")
        else:
            N.check(N.lib.msi_perspective_plane_sweep_f32(ref_faces.data_ptr(), eye.data_ptr(), kf.data_ptr(), depths.data_ptr(), 6 * b, s, s, nd,
                                                          psv.data_ptr(), 6 * nd, 0, self._stream()), "msi_perspective_plane_sweep_f32")
            N.check(N.lib.msi_cube_plane_sweep_f32(pano.data_ptr(), face_src.data_ptr(), kf.data_ptr(), depths.data_ptr(), b, hp, wp, s, nd,
                                                   psv.data_ptr(), 6 * nd, 3 * nd, self._stream()), "msi_cube_plane_sweep_f32")
        return psv

    def infer_cube(self, raw_src_equirect, raw_ref_equirect, src_pose, face_size, planes, face_intrinsics=None,
                   layer_format='f32', ngf=64, extra_outputs='', which_color_pred='blend_psv', src_sampling='face'):
        """A 360-degree pair through the PP network, face by face: preprocess both panoramas [B,H,W,3], equirect_to_cube each,
        view the faces as a batch [6B,S,S,3], format_network_input with ref_pose = I and src_pose =
        cubemap.face_poses(src_pose) (src_pose [4,4] or [B,4,4]: the source camera in the cube frame = the reference
        camera's frame), then infer_layers.  Returns the pred dict; its stack (pred['rgba_layers'] [6B,S,S,D,4] and / or
        pred['packed_layers'], which carries `planes`) goes straight into cube_render_views.  For input_type='PP' models only.
        The panoramas are single-centre equirectangular images: the faces of an ODS panorama are not perspective images.
        src_sampling: 'face' (the default) sweeps each face's own source image with the reference's wrap-around sampler --
        nothing is fetched across a cube edge: a plane point that projects past the face's border gets the opposite side of
        the same face.  'panorama' fetches across edges: the source panorama is preprocessed and never cut into faces, and
        format_cube_input samples it along every plane point's own direction (the interior of a face agrees with 'face' up to
        the resampling of the cut)."""
        if self.input_type != 'PP':
            raise ValueError("infer_cube runs the perspective (PP) network on cube faces: build the model with input_type='PP'")
        panorama = self._src_sampling("infer_cube", src_sampling)
        src, ref = self.preprocess_image(raw_src_equirect), self.preprocess_image(raw_ref_equirect)
        src_faces, ref_faces, eye, face_src, kf = self._cube_faces("infer_cube", src, ref, src_pose, face_size, face_intrinsics, cut_src=not panorama)
        if panorama:
            net_input = self.format_cube_input(ref_faces, src, face_src, planes, kf)
        else:
            net_input = self.format_network_input(ref_faces, src_faces, eye, face_src, planes, kf, ref_pose_inv=eye)
        pred = self.infer_layers(net_input, len(planes), ngf, extra_outputs, which_color_pred, layer_format=layer_format)
        return self._carrying(pred, planes)

    def _cube_faces(self, who, src, ref, src_pose, face_size, face_intrinsics, cut_src=True):
        """What infer_cube and hres_cube_layers make of a pair of panoramas [B,H,W,3] (fp32, on the device): both cut into faces
        [6B,S,S,3] (equirect_to_cube), ref_pose = I and src_pose = cubemap.face_poses(src_pose) per face [6B,4,4], and the face
        camera per face [6B,3,3] -> (src_faces, ref_faces, eye, face_src, kf).  Cut faces are what src_sampling='face' sweeps,
        face by face, nothing fetched across a cube edge; src_sampling='panorama' fetches across edges from the source panorama
        itself and passes cut_src=False: src_faces is None, the source panorama is not cut."""
        from . import cubemap
        s = int(face_size)
        if src.dim() != 4 or src.shape[-1] != 3 or src.shape != ref.shape:
            raise ValueError("%s: the panoramas must be [B,H,W,3] and agree" % who)
        b = src.shape[0]
        k = cubemap.default_face_intrinsics(s) if face_intrinsics is None else face_intrinsics
        src_faces = self.equirect_to_cube(src, s, k).reshape(6 * b, s, s, 3) if cut_src else None
        ref_faces = self.equirect_to_cube(ref, s, k).reshape(6 * b, s, s, 3)
        sp = self._f32(src_pose).reshape(-1, 4, 4)
        if sp.shape[0] == 1 and b > 1:
            sp = sp.expand(b, 4, 4)
        if sp.shape[0] != b:
            raise ValueError("%s: src_pose must be [4,4] or [B,4,4] with B = %d" % (who, b))
        face_src = cubemap.face_poses(sp).reshape(6 * b, 4, 4).contiguous()
        eye = torch.eye(4, dtype=torch.float32, device=self.device).expand(6 * b, 4, 4).contiguous()
        kf = self._f32(k).reshape(-1, 3, 3)
        if kf.shape[0] not in (1, b):
            raise ValueError("%s: face_intrinsics must be [3,3] or [B,3,3] with B = %d" % (who, b))
        kf = kf.expand(b, 3, 3)[:, None].expand(b, 6, 3, 3).reshape(6 * b, 3, 3).contiguous()
        return src_faces, ref_faces, eye, face_src, kf

    def hres_cube_layers(self, blend_weights, alphas, raw_hres_src_equirect, raw_hres_ref_equirect, src_pose, face_size, planes,
                         face_intrinsics=None, layer_format='rgba8', sparse=False, src_sampling='face'):
        """The high-res stack of a cube, for cube_render_views: blend_weights / alphas [6B,S,S,D] of infer_cube(extra_outputs=
        'blend_weights alphas') and the pair of high-res panoramas [B,H,W,3] (uint8 [0,255] or float [0,1]) -> six face stacks of
        face_size per sample.  Pure composition: the raw panoramas are cut into faces [6B,face_size,face_size,3] in [0,1]
        (equirect_to_cube), with the face poses of infer_cube and face_intrinsics ([3,3] or [B,3,3], default
        cubemap.default_face_intrinsics(face_size): those of the HIGH-RES faces), and mpi_hres_layers (sparse=False: its result
        dict) or mpi_hres_layers_sparse (sparse=True: {'sparse_layers': SparseLayers}, face_size % 16 == 0) builds the stack of
        batch 6B, which goes straight into cube_render_views.  layer_format as there.  Packed is the default here: the viewer
        refuses a sample whose six fp32 face stacks reach 2^31 bytes (face_size > 836 at D = 32; 1182 in rgba16f, 1672 in rgba8).
        Any model.  src_sampling='face' (the default): the background comes from each face's own cut source image, face by face
        -- nothing is fetched across a cube edge.  src_sampling='panorama' fetches across edges: the source panorama is not cut,
        and the background taps of every texel come from the panorama along the plane point's own direction, in one launch
        (msi_cube_hres_layers / msi_cube_hres_layers_sparse): the bits of format_cube_input at face_size ->
        msi_resize_bilinear_f32 -> msi_assemble_rgba_scaled_f32, packed or sparse as in 'face' mode."""
        panorama = self._src_sampling("hres_cube_layers", src_sampling)
        to_unit = lambda x: (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.device)
        src, ref = to_unit(raw_hres_src_equirect), to_unit(raw_hres_ref_equirect)
        src, ref = (x.float() / 255.0 if x.dtype == torch.uint8 else x.float() for x in (src, ref))
        src_faces, ref_faces, eye, face_src, kf = self._cube_faces("hres_cube_layers", src, ref, src_pose, face_size, face_intrinsics,
                                                                   cut_src=not panorama)
        if panorama:
            return self._cube_hres_build(blend_weights, alphas, self.preprocess_image(ref_faces), self.preprocess_image(src), face_src, planes, kf,
                                         sparse, *self._layer_formats(layer_format))
        build = self.mpi_hres_layers_sparse if sparse else self.mpi_hres_layers
        return build(blend_weights, alphas, ref_faces, src_faces, eye, face_src, planes, kf, ref_pose_inv=eye, layer_format=layer_format)

    def _cube_hres_build(self, blend_weights, alphas, ref_faces, src_panorama, face_src_poses, planes, face_intrinsics, sparse, want_f32, pfmt):
        """hres_cube_layers(src_sampling='panorama'): _hres_dense / _hres_sparse with the cube entry points.  ref_faces [6B,S,S,3] and
        src_panorama [B,Hp,Wp,3] are preprocessed ([-1,1]); (want_f32, pfmt) = _layer_formats of the caller's request."""
        who = "hres_cube_layers"
        ref_faces, pano, eye, face_src, kf, b, s = self._cube_sweep_inputs(who, ref_faces, src_panorama, face_src_poses, face_intrinsics)
        bw, al = self._f32(blend_weights), self._f32(alphas)
        if bw.dim() != 4 or bw.shape != al.shape or bw.shape[0] != 6 * b or bw.shape[1] != bw.shape[2]:
            raise ValueError("%s: blend_weights and alphas must be [6B,s,s,D] with 6B = %d and agree" % (who, 6 * b))
        low, d = bw.shape[1], bw.shape[3]
        depths = self._depths(planes, d)
        hp, wp = pano.shape[1], pano.shape[2]
        head = (ref_faces.data_ptr(), pano.data_ptr(), eye.data_ptr(), face_src.data_ptr(), kf.data_ptr(), depths.data_ptr(), bw.data_ptr(),
                al.data_ptr(), b, hp, wp, low, s, d)
        if not sparse:
            return self._hres_dense("msi_cube_hres_layers", head, (6 * b, d, s, s), planes, want_f32, pfmt)
        if want_f32 or pfmt is None:
            raise ValueError("%s: sparse=True takes layer_format 'rgba8' or 'rgba16f' alone (fp32 pools are not built)" % who)
        return self._hres_sparse("msi_hres_index_tiles_edge", "msi_cube_hres_layers_sparse", head, al, (low, low), (6 * b, d, s, s), planes, pfmt, 'edge')

    # ------------------------------------------------------------------ image scores (eval.py:127-174 on the device)
    SCORE_TRANSFORMS = {'raw': N.MSI_SCORE_RAW, 'image': N.MSI_SCORE_IMAGE, 'depth': N.MSI_SCORE_DEPTH}
    SCORE_METRICS = {'mse': N.MSI_SCORE_MSE, 'psnr': N.MSI_SCORE_MSE, 'mae': N.MSI_SCORE_MAE, 'ssim': N.MSI_SCORE_SSIM}

    def score_views(self, pred, target, metrics=('psnr', 'ssim', 'mae'), transform='image', quantize=True, row_weights=None,
                    max_val=255.0):
        """PSNR / SSIM / mean absolute difference of images that are on the device (msi_score_images; evaluate.py states the
        same numbers on the host) -> dict of float64 device tensors of shape L, one entry per requested metric and always 'mse'.

        pred [*L,h,w,C] and target [*P,h,w,C], C in 1..4, both fp32 or both uint8, both on this model's device; P is a prefix
        of L, and every pred image is scored against the target image of its leading P indices: [B,V,h,w,C] renders against
        [B,h,w,C] ground truth, or any batch against one [h,w,C] image.
        transform: what a stored value means -- 'image' ([-1,1] -> 0..255, deprocess_image's range), 'depth' ([0,1] -> 0..255)
        or 'raw' (the value as it is); quantize=True scores the 8-bit level deprocess_image / deprocess_depth_image would
        store (what the harness writes to PNG), False the unrounded value; 'raw' values have no level, quantize is ignored
        for them.  uint8 images are levels already: 'raw', no quantisation, whatever these two arguments say.
        row_weights: None, 'solid_angle' (evaluate.solid_angle_row_weights(h): WS-PSNR and its SSIM / MAE counterparts for
        equirectangular images) or h weights; msi_hip.h gives the weighted formulas.
        fp64 on the device, bit-reproducible; the workspace is allocated per call and nothing synchronises."""
        if not (torch.is_tensor(pred) and torch.is_tensor(target)):
            raise TypeError("score_views: pred and target must be torch tensors on %s" % (self.device,))
        if pred.device != self.device or target.device != self.device:
            raise ValueError("score_views: pred is on %s and target on %s, the model on %s" % (pred.device, target.device, self.device))
        if pred.dtype != target.dtype or pred.dtype not in (torch.float32, torch.uint8):
            raise TypeError("score_views: pred and target must both be float32 or both uint8, got %s and %s" % (pred.dtype, target.dtype))
        ps, ts = tuple(pred.shape), tuple(target.shape)
        if len(ps) < 3 or len(ts) < 3 or len(ts) > len(ps) or ps[-3:] != ts[-3:] or ts[:-3] != ps[:len(ts) - 3]:
            raise ValueError("score_views: pred %s and target %s must be [*L,h,w,C] and [*P,h,w,C] with P a prefix of L" % (ps, ts))
        h, w, c = ps[-3:]
        lead = ps[:-3]
        n_pairs = int(np.prod(lead, dtype=np.int64)) if lead else 1
        n_targets = int(np.prod(ts[:-3], dtype=np.int64)) if len(ts) > 3 else 1
        if n_pairs < 1 or min(h, w) < 1 or not 1 <= c <= 4:
            raise ValueError("score_views: empty batch or image, or C outside 1..4: pred %s, target %s" % (ps, ts))
        metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
        unknown = [m for m in metrics if m not in self.SCORE_METRICS]
        if unknown:
            raise ValueError("score_views: unknown metrics %s (of %s)" % (unknown, sorted(self.SCORE_METRICS)))
        mask = N.MSI_SCORE_MSE
        for m in metrics:
            mask |= self.SCORE_METRICS[m]
        if (mask & N.MSI_SCORE_SSIM) and min(h, w) < 11:
            raise ValueError("score_views: SSIM needs images of at least 11 x 11, got %d x %d (pred %s)" % (h, w, ps))
        if pred.dtype == torch.uint8:
            dtype, tcode, q = N.MSI_SCORE_U8, N.MSI_SCORE_RAW, 0
        else:
            if transform not in self.SCORE_TRANSFORMS:
                raise ValueError("score_views: transform must be one of %s" % sorted(self.SCORE_TRANSFORMS))
            dtype, tcode = N.MSI_SCORE_F32, self.SCORE_TRANSFORMS[transform]
            q = int(bool(quantize) and tcode != N.MSI_SCORE_RAW)
        weights = None
        if row_weights is not None:
            if isinstance(row_weights, str):
                if row_weights != 'solid_angle':
                    raise ValueError("score_views: row_weights must be None, 'solid_angle' or %d weights" % h)
                from .evaluate import solid_angle_row_weights
                row_weights = solid_angle_row_weights(h)
            if not torch.is_tensor(row_weights):
                row_weights = torch.as_tensor(np.asarray(row_weights, dtype=np.float64))
            weights = row_weights.to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
            if weights.numel() != h:
                raise ValueError("score_views: %d row weights for images of %d rows (pred %s)" % (weights.numel(), h, ps))
        pred, target = pred.contiguous(), target.contiguous()
        out = torch.empty((n_pairs, 4), dtype=torch.float64, device=self.device)
        ws_bytes = N.lib.msi_score_workspace_bytes(n_pairs, h, w, c)
        if ws_bytes == 0:
            raise N.MsiError("msi_score_workspace_bytes failed: %s" % N.last_error())
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        N.check(N.lib.msi_score_images(pred.data_ptr(), target.data_ptr(), dtype, tcode, q, n_pairs, n_pairs // n_targets, h, w, c,
                                       _ptr(weights), float(max_val), mask, out.data_ptr(), ws.data_ptr(), ws_bytes, self._stream()),
                "msi_score_images")
        cols = {'mse': 0, 'mae': 1, 'ssim': 2, 'psnr': 3}
        return {m: out[:, cols[m]].reshape(lead) for m in ('mse',) + tuple(m for m in metrics if m != 'mse')}

    def score_consecutive(self, frames, transform='image', quantize=True):
        """Mean absolute difference of neighbouring frames, [N,h,w,C] -> [N-1] float64 on the device: the quantity of
        evaluate.evaluate_consecutive_one (eval.py:147-174) without the files.  transform / quantize as in score_views."""
        if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[0] < 2:
            raise ValueError("score_consecutive: frames must be a [N,h,w,C] tensor with N >= 2, got %s" %
                             (tuple(frames.shape) if torch.is_tensor(frames) else type(frames),))
        frames = frames.contiguous()
        return self.score_views(frames[:-1], frames[1:], metrics=('mae',), transform=transform, quantize=quantize)['mae']
