"""numpy / Pillow restatement of the letterboxed detector input (csrc/letterbox.hip) and of the box un-mapping (csrc/post.hip,
yolo_compact_k<true>): the definitions the kernels are held to, bit for bit.

Geometry -- the reference's letterbox_image (yolo3/utils.py:18-28 = tools/yolo.py:141-151), Python floats (f64) and int() truncation:
    s = min(w * 1.0 / W, h * 1.0 / H);  new_w = int(W * s);  new_h = int(H * s);  offset = ((w - new_w) // 2, (h - new_h) // 2)
Pixels -- Pillow itself:
    Image.new('RGB', (w, h), (pad,) * 3).paste(Image.fromarray(rgb).resize((new_w, new_h), Image.LANCZOS), (off_x, off_y))
Boxes -- the shape of tools/yolo.py:78-86 (correct_yolo_boxes) in f64, in this order, rounded once to f32, with the INTEGER paste offset
(where the pixels are; the reference divides by 2.), no int() and no clipping:
    X = (x - off_x / net_w) / (new_w / net_w) * W        Y = (y - off_y / net_h) / (new_h / net_h) * H
x, y being the f32 corners cx -+ bw / 2, cy -+ bh / 2 of a row, formed in f32."""
import numpy as np

LDS_BUDGET = 64 * 1024           # letterbox_lanczos_k's band of rows (csrc/letterbox.hip LB_LDS_BUDGET)


def geometry(W, H, net_w, net_h):
    """-> (new_w, new_h, off_x, off_y); ValueError where Pillow's resize would raise it (a picture without width or height)."""
    s = min(net_w * 1.0 / W, net_h * 1.0 / H)
    new_w, new_h = int(W * s), int(H * s)
    if new_w <= 0 or new_h <= 0:
        raise ValueError('height and width must be > 0')
    return new_w, new_h, (net_w - new_w) // 2, (net_h - new_h) // 2


def canvas(rgb, net_w, net_h, pad):
    """rgb u8 [H, W, 3] -> the letterboxed canvas u8 [net_h, net_w, 3]."""
    from PIL import Image
    H, W = rgb.shape[:2]
    new_w, new_h, off_x, off_y = geometry(W, H, net_w, net_h)
    out = Image.new('RGB', (net_w, net_h), (pad,) * 3)
    out.paste(Image.fromarray(np.ascontiguousarray(rgb)).resize((new_w, new_h), Image.LANCZOS), (off_x, off_y))
    return np.asarray(out)


def lanczos_window(in_size, out_size, xx):
    """(first source index, taps) of output xx: the bounds of Pillow's precompute_coeffs for the Lanczos filter (support 3)."""
    scale = in_size / out_size
    support = 3.0 * max(scale, 1.0)
    center = (xx + 0.5) * scale
    lo = max(int(center - support + 0.5), 0)
    return lo, min(int(center + support + 0.5), in_size) - lo


def one_row_window_bytes(W, H, net_w, net_h):
    """LDS bytes the one-launch kernel needs for a band of ONE canvas row: the rows of the widest vertical window, new_w * 3 bytes each,
    every row starting at the canvas's 16-byte phase and padded to 16.  Above LDS_BUDGET the geometry takes the two-launch form."""
    new_w, new_h, off_x, _ = geometry(W, H, net_w, net_h)
    pitch = (off_x * 3 % 16 + new_w * 3 + 15) // 16 * 16
    rows = max(lanczos_window(H, new_h, yy)[1] for yy in range(new_h)) if new_h != H else 1
    return rows * pitch


def unmap_corners(v, offset, new, net, size):
    """f32 canvas-normalised corner coordinates -> f32 frame pixels along one axis."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    a = np.float64(offset) / np.float64(net)
    b = np.float64(new) / np.float64(net)
    return (((v - a) / b) * np.float64(size)).astype(np.float32)


def decode(raw, thr, W, H, net_w, net_h):
    """tools/yolov5.py:120-131 on raw f32 [rows, 5 + classes] with the un-mapping above in place of `* W`, `* H`:
    -> (boxes f32 [n, 4] xyxy frame pixels, scores f32 [n], classes int [n]) of the rows with confidence >= thr, in row order."""
    raw = np.asarray(raw, dtype=np.float32)
    new_w, new_h, off_x, off_y = geometry(W, H, net_w, net_h)
    prod = raw[:, 5:] * raw[:, 4:5]                                # f32
    cls = np.argmax(prod, axis=1)
    conf = np.take_along_axis(prod, cls[:, None], axis=1)[:, 0]
    keep = np.where(conf >= np.float32(thr))[0]
    x, y, bw, bh = (raw[keep, i] for i in range(4))
    two = np.float32(2)
    x1, y1, x2, y2 = x - bw / two, y - bh / two, x + bw / two, y + bh / two      # f32, as yolo_compact_k forms them
    boxes = np.stack([unmap_corners(x1, off_x, new_w, net_w, W), unmap_corners(y1, off_y, new_h, net_h, H),
                      unmap_corners(x2, off_x, new_w, net_w, W), unmap_corners(y2, off_y, new_h, net_h, H)], axis=1)
    return boxes, conf[keep], cls[keep].astype(np.int32)
