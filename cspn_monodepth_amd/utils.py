"""The picture half of the reference's `libs.utils` on the device — the drop-in for the comparison sheet of `trainer.eval`
(libs/trainers/single_gpu_trainer.py:140-175 calling libs/utils.py:69-192):

    from cspn_monodepth_amd import utils                          # was: from libs import utils

`colored_depthmap`, `merge_into_row`, `merge_into_row_with_gt`, `merge_rgb_depth_into_row`, `add_row`, `save_image`,
`feature_map`, `merge_features_into_row`, `add_features_row`, `save_featues_map` (the reference's own spelling) and
`save_features` keep the reference's argument order.  They take DEVICE tensors and return a device `uint8 [H, P * W, 3]` tensor:
two launches of include/cspn_visual.h on the current stream, no host synchronisation, capturable in a graph.  The bytes are those
the reference's float64 array becomes in `save_image` (`astype('uint8')`), held to it by golden G25.

Two deliberate differences:
  * the return value is uint8, not float64 — `save_image` casts to uint8 anyway, and nothing else reads the array;
  * RGB outside [0, 256) after scaling, where numpy's cast is platform-defined, SATURATES (NaN gives 0).
Reproduced on purpose: `merge_into_row` and `merge_rgb_depth_into_row` do not scale RGB by 255 (libs/utils.py:79-80), so an RGB
panel of [0, 1] values comes out as bytes 0 and 1; `merge_into_row_with_gt` does scale.  A uint8 RGB tensor is copied as it is.

`comparison_rows(input, target, pred, modality)` is the batched form, `[B, H, P * W, 3]` in two launches.  `ComparisonSheet`
collects the reference's 8 rows in one preallocated `[rows * H, P * W, 3]` device buffer — the kernel writes each row in place —
and copies to the host once, in `save()`.

Refused with an error instead of converting: CPU tensors, any depth dtype but fp32, planes that are not contiguous (a channel or
batch slice of a contiguous tensor is fine), panels whose H x W differ.  The reference resizes `pred` with `F.interpolate` before
it draws; that stays a stock op in the caller.

Left out: `get_save_path`, `get_logger`, `write_config_file`, `save_checkpoint` — file-system housekeeping around the run, and
`get_logger` needs tensorboardX.  PIL is imported only inside `save_image` / `save_features` / `ComparisonSheet.save`."""
import torch

from . import _lib
from ._host import _p, launch

__all__ = ["colored_depthmap", "merge_into_row", "merge_into_row_with_gt", "merge_rgb_depth_into_row", "add_row", "save_image",
           "feature_map", "merge_features_into_row", "add_features_row", "save_featues_map", "save_features", "comparison_rows",
           "ComparisonSheet", "workspace_bytes"]


def workspace_bytes(B, n_planes, elements):
    """Bytes of workspace for B frames of n_planes range units of `elements` elements (needs no device)."""
    n = _lib.lib().cspn_visual_workspace_bytes(int(B), int(n_planes), int(elements))
    _lib.check(n, "cspn_visual_workspace_bytes")
    return n


def _device_of(tensors):
    devices = {t.device for t in tensors}
    for t in tensors:
        if t.device.type != "cuda":
            raise RuntimeError("utils: tensors must live on a ROCm device, got %s (no CPU implementation here)" % t.device)
    if len(devices) > 1:
        raise RuntimeError("utils: tensors on more than one device (%s)" % ", ".join(sorted(str(d) for d in devices)))
    return next(iter(devices))


def _planes(t, what, channels):
    """t as [B, channels, H, W] with contiguous H x W planes (unit axes are added in front, as the reference squeezes them away);
    -> (tensor, frame stride, channel stride) in elements."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("utils: %s must be a tensor, got %s" % (what, type(t).__name__))
    t = t.detach()
    lead = 3 if channels else 2                    # dims of one frame: [C, H, W] or [H, W]
    if channels is None and t.dim() >= 3 and t.shape[-3] == 1:
        t = t.squeeze(-3)
    while t.dim() < lead + 1:
        t = t.unsqueeze(0)
    if t.dim() != lead + 1:
        raise RuntimeError("utils: %s of shape %s" % (what, tuple(t.shape)))
    if channels and t.shape[1] != channels:
        raise RuntimeError("utils: %s must have %d channels, got shape %s" % (what, channels, tuple(t.shape)))
    H, W = t.shape[-2], t.shape[-1]
    ok = (W == 1 or t.stride(-1) == 1) and (H == 1 or t.stride(-2) == W)
    if not ok:
        raise RuntimeError("utils: %s has non-contiguous planes (shape %s, strides %s)" % (what, tuple(t.shape), tuple(t.stride())))
    return t, t.stride(0), (t.stride(1) if channels else 0)


def _depth(t, what):
    if isinstance(t, torch.Tensor) and t.dtype != torch.float32:
        raise RuntimeError("utils: %s must be fp32, got %s (no other dtype is built)" % (what, t.dtype))
    return _planes(t, what, None)


def _rgb(t):
    if isinstance(t, torch.Tensor) and t.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError("utils: the RGB input must be fp32 or uint8, got %s" % (t.dtype,))
    return _planes(t, "the RGB input", 3)


def _out(out, B, H, row_pixels, device):
    if out is None:
        return torch.empty((B, H, row_pixels, 3), dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or out.device != device or not out.is_contiguous() or out.numel() != B * H * row_pixels * 3 \
            or tuple(out.shape[-2:]) != (row_pixels, 3):
        raise RuntimeError("utils: out must be a contiguous uint8 tensor [%d, %d, %d, 3] (or [%d, %d, 3]) on %s, got %s %s on %s"
                           % (B, H, row_pixels, B * H, row_pixels, device, tuple(out.shape), out.dtype, out.device))
    return out


def _rows(rgb, scale, depths, d_min=None, d_max=None, out=None, work=None):
    """The call behind every row form: rgb (None or a tensor), depths in argument order -> uint8 [B, H, P * W, 3]."""
    planes = [_depth(d, "depth plane %d" % k) for k, d in enumerate(depths)]
    tensors = [p[0] for p in planes]
    rgbp = None
    if rgb is not None:
        rgbp = _rgb(rgb)
        tensors.append(rgbp[0])
    device = _device_of(tensors)
    B, H, W = tensors[0].shape[0], tensors[0].shape[-2], tensors[0].shape[-1]
    for t in tensors[1:]:
        if (t.shape[0], t.shape[-2], t.shape[-1]) != (B, H, W):
            raise RuntimeError("utils: panels of %s and %s — every panel must have the same B x H x W (resize the prediction first, as "
                               "the reference does with F.interpolate)" % (tuple(tensors[0].shape), tuple(t.shape)))
    if B * H * W == 0:
        raise RuntimeError("utils: empty planes of shape %s" % (tuple(tensors[0].shape),))
    a = _lib.cspn_visual_rows()
    if rgbp is not None:
        a.rgb, a.rgb_frame_stride, a.rgb_channel_stride = rgbp[0].data_ptr(), rgbp[1], rgbp[2]
        a.rgb_kind = _lib.VISUAL_RGB_U8 if rgbp[0].dtype == torch.uint8 else _lib.VISUAL_RGB_F32
    else:
        a.rgb_kind = _lib.VISUAL_RGB_NONE
    a.rgb_scale = float(scale)
    a.n_depth = len(planes)
    for k, (t, fs, _) in enumerate(planes):
        a.depth[k], a.depth_frame_stride[k] = t.data_ptr(), fs
    a.use_min, a.use_max = int(d_min is not None), int(d_max is not None)
    a.d_min, a.d_max = float(d_min or 0.0), float(d_max or 0.0)
    P = len(planes) + (rgbp is not None)
    out = _out(out, B, H, P * W, device)
    if work is None and not (a.use_min and a.use_max):
        work = torch.empty(workspace_bytes(B, len(planes), H * W), dtype=torch.uint8, device=device)
    launch(device, "cspn_visual_rows", a, B, H, W, out.data_ptr(), H * P * W * 3, _p(work))
    return out.view(B, H, P * W, 3)


def _features(features, n, out=None):
    if isinstance(features, torch.Tensor) and features.dtype != torch.float32:
        raise RuntimeError("utils: features must be fp32, got %s (no other dtype is built)" % (features.dtype,))
    if not isinstance(features, torch.Tensor):
        raise TypeError("utils: features must be a tensor, got %s" % type(features).__name__)
    f = features.detach()
    while f.dim() > 3 and f.shape[0] == 1:
        f = f.squeeze(0)
    if f.dim() != 3:
        raise RuntimeError("utils: features of shape %s, expected [C, H, W]" % (tuple(features.shape),))
    device = _device_of([f])
    if not f.is_contiguous():
        raise RuntimeError("utils: features are not contiguous (shape %s, strides %s)" % (tuple(f.shape), tuple(f.stride())))
    C, H, W = f.shape
    n = int(n)
    if not 1 <= n <= C or H * W == 0:
        raise RuntimeError("utils: %d feature panels of a tensor of shape %s" % (n, tuple(f.shape)))
    out = _out(out, 1, H, n * W, device)
    work = torch.empty(workspace_bytes(1, 1, C * H * W), dtype=torch.uint8, device=device)
    launch(device, "cspn_visual_features", f.data_ptr(), C * H * W, 1, C, H, W, n, out.data_ptr(), H * n * W * 3, work.data_ptr())
    return out.view(H, n * W, 3)


def _single(rows):
    if rows.shape[0] != 1:
        raise RuntimeError("utils: this form draws one frame, got a batch of %d (comparison_rows is the batched form)" % rows.shape[0])
    return rows[0]


# ------------------------------------------------------------------------------------------------ libs/utils.py, name for name
def colored_depthmap(depth, d_min=None, d_max=None):
    """[H, W] fp32 -> uint8 [H, W, 3]; d_min / d_max as given (rounded to fp32) or the plane's own."""
    return _single(_rows(None, 1.0, [depth], d_min, d_max))


def merge_into_row(input, depth_target, depth_pred):
    return _single(_rows(input, 1.0, [depth_target, depth_pred]))


def merge_into_row_with_gt(input, depth_input, depth_target, depth_pred):
    return _single(_rows(input, 255.0, [depth_input, depth_target, depth_pred]))


def merge_rgb_depth_into_row(input, depth):
    return _single(_rows(input, 1.0, [depth]))


def add_row(img_merge, row):
    return torch.cat([img_merge, row], 0)


def _to_image(img_merge):
    from PIL import Image
    if isinstance(img_merge, torch.Tensor):
        img_merge = img_merge.cpu().numpy()
    return Image.fromarray(img_merge.astype("uint8"))


def save_image(img_merge, filename):
    _to_image(img_merge).save(filename)


def feature_map(feature, min=None, max=None):
    return _single(_rows(None, 1.0, [feature], min, max))


def merge_features_into_row(features, featuers_num=9):
    """[C, H, W] -> uint8 [H, featuers_num * W, 3]: one range over ALL C planes, as the reference's np.min(features)."""
    return _features(features, featuers_num)


def add_features_row(img_merge, row):
    return torch.cat([img_merge, row], 0)


def save_featues_map(img_merge, name):
    _to_image(img_merge).save(name)


def save_features(features, filename, features_num=9):
    _to_image(_features(features, features_num)).save(filename)


# ------------------------------------------------------------------------------------------------ batched forms
def _split(input, modality):
    if modality not in ("rgb", "rgbd"):
        raise ValueError("utils: modality %r has no comparison image (the reference draws none for 'd')" % (modality,))
    channels = 3 if modality == "rgb" else 4
    if not isinstance(input, torch.Tensor) or input.dim() != 4 or input.shape[1] != channels:
        raise RuntimeError("utils: modality %r takes an input of shape [B, %d, H, W], got %s"
                           % (modality, channels, tuple(input.shape) if isinstance(input, torch.Tensor) else type(input).__name__))
    return (input, None) if modality == "rgb" else (input[:, :3], input[:, 3:])


def comparison_rows(input, target, pred, modality, out=None, work=None):
    """The rows `trainer.eval` draws, for a whole batch: input [B, 3 or 4, H, W], target and pred [B, 1, H, W] ->
    uint8 [B, H, P * W, 3] with P = 3 ('rgb': merge_into_row) or 4 ('rgbd': merge_into_row_with_gt, the sparse input first).
    out: a contiguous uint8 tensor of that size to write into (a slice of a larger buffer, for instance)."""
    rgb, sparse = _split(input, modality)
    if sparse is None:
        return _rows(rgb, 1.0, [target, pred], out=out, work=work)
    return _rows(rgb, 255.0, [sparse, target, pred], out=out, work=work)


class ComparisonSheet(object):
    """The reference's comparison sheet: `rows` frames (8 in trainer.eval) stacked in one device buffer [rows * H, P * W, 3].

        sheet = ComparisonSheet(8, "rgb")
        for i, (input, target) in enumerate(loader):
            ...
            if i % skip == 0 and not sheet.full:
                sheet.add(input[0], target[0], pred[0])           # two launches, written in place
        sheet.save(path)                                          # the only copy to the host

    The buffer and the workspace are allocated by the first `add` (or by `reserve(H, W, device)`, ahead of a graph capture);
    later frames must have its H x W.  `add` returns the row's index; a full sheet refuses further rows."""

    def __init__(self, rows=8, modality="rgb"):
        if modality not in ("rgb", "rgbd"):
            raise ValueError("ComparisonSheet: modality %r has no comparison image" % (modality,))
        if int(rows) < 1:
            raise ValueError("ComparisonSheet: rows %r" % (rows,))
        self.rows, self.modality, self.panels = int(rows), modality, 3 if modality == "rgb" else 4
        self.filled, self.buffer, self.work, self.H, self.W = 0, None, None, None, None

    @property
    def full(self):
        return self.filled >= self.rows

    def reserve(self, H, W, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("ComparisonSheet: the sheet lives on a ROCm device, got %s" % device)
        if self.buffer is not None:
            if (self.H, self.W) != (H, W) or self.buffer.device != device:
                raise RuntimeError("ComparisonSheet: a frame of %d x %d on %s for a sheet of %d x %d on %s"
                                   % (H, W, device, self.H, self.W, self.buffer.device))
            return self
        nbytes = workspace_bytes(1, self.panels - 1, H * W)
        self.H, self.W = int(H), int(W)
        self.buffer = torch.zeros((self.rows * H, self.panels * W, 3), dtype=torch.uint8, device=device)
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self

    def row_slice(self, index):
        """The rows of frame `index` in the sheet: buffer[index * H : (index + 1) * H]."""
        if not 0 <= index < self.rows:
            raise IndexError("ComparisonSheet: row %d of %d" % (index, self.rows))
        return slice(index * self.H, (index + 1) * self.H)

    def add(self, input, target, pred, index=None):
        """One frame: input [3 or 4, H, W], target and pred [1, H, W].  index: the row to (over)write, default the next free one."""
        if input.dim() == 3:
            input = input.unsqueeze(0)
        if input.shape[0] != 1:
            raise RuntimeError("ComparisonSheet.add takes one frame, got a batch of %d" % input.shape[0])
        k = self.filled if index is None else int(index)
        if k >= self.rows or k < 0:
            raise RuntimeError("ComparisonSheet: the sheet holds %d rows" % self.rows)
        _split(input, self.modality)
        self.reserve(input.shape[-2], input.shape[-1], input.device)
        comparison_rows(input, target, pred, self.modality, out=self.buffer[self.row_slice(k)], work=self.work)
        if index is None:
            self.filled += 1
        return k

    def image(self):
        """The filled part of the sheet, uint8 [filled * H, P * W, 3], on the device (a view)."""
        if self.buffer is None:
            raise RuntimeError("ComparisonSheet: nothing was added")
        return self.buffer[:self.filled * self.H]

    def save(self, filename):
        save_image(self.image(), filename)
