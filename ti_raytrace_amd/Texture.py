"""Environment / albedo texture (mirror of the reference's ``texture/Texture.py``).

The reference loads with ``cv2.imread`` (BGR, alpha dropped) and packs each texel into one
i32 ``0xRRGGBB`` stored x-major with y flipped (``texture/Texture.py:18-34``).  cv2 is not
available here; PIL's ``convert('RGB')`` yields the same 8-bit channels.  Sampling
(``sample`` / ``texture2D``, :41-69) runs on the device inside the miss branch of
``PT_RGB.render``.

Extension (no reference counterpart; include/tirt.h, "HDR environment"): an environment of RGBE8 texels
``(E << 24) | (R << 16) | (G << 8) | B``, a channel being ``mantissa * 2^(E - 136)`` of linear radiance --
from a Radiance ``.hdr`` file (``load_hdr``, whose bytes go to the texels unchanged) or from a float array
(``load_array_float``, a stated encoder).  ``format`` says which of the two packings ``np_img`` holds.
"""
import numpy as np

FORMAT_RGB8, FORMAT_RGBE8 = 0, 1


class Texture:
    def __init__(self):
        self.wid = 0
        self.hgt = 0
        self.channel = 0
        self.size = 0
        self.np_img = None
        self.format = FORMAT_RGB8

    def load_image(self, imagePath):
        from PIL import Image
        img = np.asarray(Image.open(imagePath).convert("RGB"), dtype=np.int32)   # [hgt, wid, 3] RGB
        self.load_array(img)

    def load_array(self, rgb_u8):
        """rgb_u8: [hgt, wid, 3] integer array, row 0 = top of the image."""
        img = np.asarray(rgb_u8).astype(np.int32)
        self.format = FORMAT_RGB8
        self.hgt, self.wid, self.channel = img.shape[0], img.shape[1], 3
        self.size = self.wid * self.hgt * self.channel
        packed = (img[:, :, 0] << 16) | (img[:, :, 1] << 8) | img[:, :, 2]          # [hgt, wid]
        # np_img[j, hgt-1-i] = packed[i, j]   (texture/Texture.py:29-34)
        self.np_img = np.ascontiguousarray(packed[::-1, :].T, dtype=np.int32)       # [wid, hgt]

    def load_image_rgba(self, imagePath):
        """An image with its alpha channel (one without is opaque): the cut-out packing of load_array_rgba."""
        from PIL import Image
        self.load_array_rgba(np.asarray(Image.open(imagePath).convert("RGBA"), dtype=np.int32))

    def load_array_rgba(self, rgba_u8):
        """rgba_u8: [hgt, wid, 4] integer array, row 0 = top of the image.  Bits 24..31 of a texel hold 255 - A, the transparency (include/tirt.h,
        "Alpha cut-outs"): an opaque texel is the 0xRRGGBB of load_array, bit for bit."""
        img = np.asarray(rgba_u8).astype(np.int64)
        self.format = FORMAT_RGB8
        self.hgt, self.wid, self.channel = img.shape[0], img.shape[1], 4
        self.size = self.wid * self.hgt * self.channel
        packed = ((255 - img[:, :, 3]) << 24) | (img[:, :, 0] << 16) | (img[:, :, 1] << 8) | img[:, :, 2]
        self.np_img = np.ascontiguousarray(packed[::-1, :].T.astype(np.uint32).view(np.int32))       # [wid, hgt]

    def load_black(self, wid=512, hgt=512):
        """Equivalent of the reference's default ``image/black.png`` (Scene.py:295-296)."""
        self.load_array(np.zeros((hgt, wid, 3), np.int32))

    def _set_rgbe(self, rgbe_u8):
        """rgbe_u8: [hgt, wid, 4] uint8 (R, G, B, E), row 0 = top of the image.  A texel with E == 0 becomes the all-zero word (black: the only E == 0 texel
        tirt_env_upload_hdr accepts); every other texel keeps its four bytes."""
        img = np.asarray(rgbe_u8).astype(np.int64)
        self.format = FORMAT_RGBE8
        self.hgt, self.wid, self.channel = img.shape[0], img.shape[1], 3
        self.size = self.wid * self.hgt * self.channel
        packed = (img[:, :, 3] << 24) | (img[:, :, 0] << 16) | (img[:, :, 1] << 8) | img[:, :, 2]
        packed = np.where(img[:, :, 3] == 0, 0, packed)
        self.np_img = np.ascontiguousarray(packed[::-1, :].T.astype(np.uint32).view(np.int32))       # [wid, hgt], the layout of load_array

    def load_array_float(self, rgb):
        """rgb: [hgt, wid, 3] float32 / float64 linear radiance, row 0 = top of the image -> RGBE8 texels.  The encoder, per texel, exact in float64:
          m = max(r, g, b);  m < 2^-135 (the smallest value a texel can hold, mantissa 1 at E = 1): black, the all-zero word;
          otherwise E = clamp(frexp(m).exponent + 128, 1, 255)   (frexp: m = f * 2^exponent, 0.5 <= f < 1, so the largest mantissa lies in 128 .. 255 unless E was clamped)
          and each mantissa = min(255, floor(c * 2^(136 - E))).
        Encoding TRUNCATES: decode(encode(x)) <= x per channel, and the largest channel loses less than one unit of a mantissa of 128 .. 255, a relative step of
        2^-7 .. 2^-8 (smaller channels lose up to the same absolute amount; values from 2^127 up are clamped to 255 * 2^119).  A power of two on the largest
        channel is exact.  Negative, NaN or infinite input: ValueError."""
        a = np.asarray(rgb)
        if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1 or a.dtype not in (np.float32, np.float64):
            raise ValueError("Texture.load_array_float: an image array must be (h, w, 3) float32 or float64, got %s %s" % (a.dtype, a.shape))
        a = a.astype(np.float64)
        if not np.isfinite(a).all():
            raise ValueError("Texture.load_array_float: NaN or infinite radiance")
        if (a < 0).any():
            raise ValueError("Texture.load_array_float: negative radiance")
        m = a.max(axis=2)
        black = m < 2.0 ** -135
        E = np.clip(np.frexp(np.where(black, 1.0, m))[1] + 128, 1, 255).astype(np.int64)
        mant = np.minimum(255, np.floor(np.ldexp(a, (136 - E)[:, :, None]))).astype(np.int64)
        rgbe = np.concatenate([mant, E[:, :, None]], axis=2)
        rgbe[black] = 0
        self._set_rgbe(rgbe)

    def load_hdr(self, path):
        """A Radiance picture: a header whose first line starts with ``#?RADIANCE`` or ``#?RGBE`` and which names ``FORMAT=32-bit_rle_rgbe``, a blank line, the
        resolution line ``-Y h +X w`` (top row first, left to right), then h scanlines, each flat (w x 4 bytes R, G, B, E) or new-style run-length encoded
        (marker 2 2 hi lo with hi * 256 + lo == w, 8 <= w < 32768, then the w R bytes, G bytes, B bytes and E bytes each as runs: a count c > 128 repeats the
        next byte c - 128 times, 1 <= c <= 128 copies c bytes).  Anything else is a ValueError that names what was met: another signature, format (XYZE) or
        orientation, an old-style run (a flat pixel 1 1 1 n), a truncated file, a run that overruns its scanline.  The file's bytes become the texels unchanged,
        but for E == 0 texels, which become the all-zero word."""
        with open(path, "rb") as fh:
            data = fh.read()
        what = "Texture.load_hdr(%s): " % (path,)
        pos, lines = 0, []
        while True:                                                    # the header: lines up to the first empty one
            end = data.find(b"\n", pos)
            if end < 0:
                raise ValueError(what + "truncated file: the header has no end (no empty line)")
            line = data[pos:end].rstrip(b"\r")
            pos = end + 1
            if not line:
                break
            lines.append(line)
        if not lines or not (lines[0].startswith(b"#?RADIANCE") or lines[0].startswith(b"#?RGBE")):
            raise ValueError(what + "not a Radiance picture: the first line is %r, not #?RADIANCE or #?RGBE" % (lines[0][:32] if lines else b"",))
        formats = [l.split(b"=", 1)[1].strip() for l in lines[1:] if l.upper().startswith(b"FORMAT=")]
        if formats != [b"32-bit_rle_rgbe"]:
            raise ValueError(what + "FORMAT must be 32-bit_rle_rgbe, the header has %r" % (formats,))
        end = data.find(b"\n", pos)
        if end < 0:
            raise ValueError(what + "truncated file: no resolution line")
        res = data[pos:end].rstrip(b"\r").split()
        pos = end + 1
        if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X" or not res[1].isdigit() or not res[3].isdigit() or int(res[1]) < 1 or int(res[3]) < 1:
            raise ValueError(what + "only the orientation '-Y h +X w' (h, w >= 1) is read, the resolution line is %r" % (b" ".join(res),))
        h, w = int(res[1]), int(res[3])
        buf = np.frombuffer(data, np.uint8)
        out = np.zeros((h, w, 4), np.uint8)
        for row in range(h):
            if pos + 4 > buf.size:
                raise ValueError(what + "truncated file: scanline %d of %d is missing" % (row, h))
            if 8 <= w < 32768 and buf[pos] == 2 and buf[pos + 1] == 2 and buf[pos + 2] < 128:
                if (int(buf[pos + 2]) << 8 | int(buf[pos + 3])) != w:
                    raise ValueError(what + "scanline %d: the run-length marker names width %d, the picture has %d" % (row, int(buf[pos + 2]) << 8 | int(buf[pos + 3]), w))
                pos += 4
                for comp in range(4):
                    x = 0
                    while x < w:
                        if pos >= buf.size:
                            raise ValueError(what + "truncated file: scanline %d ends inside component %d" % (row, comp))
                        c = int(buf[pos]); pos += 1
                        if c > 128:
                            c -= 128
                            if x + c > w:
                                raise ValueError(what + "scanline %d, component %d: a run of %d overruns the scanline at %d of %d" % (row, comp, c, x, w))
                            if pos >= buf.size:
                                raise ValueError(what + "truncated file: scanline %d ends inside a run" % row)
                            out[row, x:x + c, comp] = buf[pos]; pos += 1
                        else:
                            if c == 0:
                                raise ValueError(what + "scanline %d, component %d: a count of 0" % (row, comp))
                            if x + c > w:
                                raise ValueError(what + "scanline %d, component %d: %d literal bytes overrun the scanline at %d of %d" % (row, comp, c, x, w))
                            if pos + c > buf.size:
                                raise ValueError(what + "truncated file: scanline %d ends inside %d literal bytes" % (row, c))
                            out[row, x:x + c, comp] = buf[pos:pos + c]; pos += c
                        x += c
            else:
                if pos + 4 * w > buf.size:
                    raise ValueError(what + "truncated file: flat scanline %d needs %d bytes, %d are left" % (row, 4 * w, buf.size - pos))
                line = buf[pos:pos + 4 * w].reshape(w, 4)
                if ((line[:, 0] == 1) & (line[:, 1] == 1) & (line[:, 2] == 1)).any():
                    raise ValueError(what + "scanline %d: a pixel 1 1 1 n, an old-style run-length repeat, which is not read" % row)
                out[row] = line; pos += 4 * w
        self._set_rgbe(out)

    def setup_data_gpu(self, ctx, power):
        if self.format == FORMAT_RGBE8:
            ctx.env_upload_hdr(self.np_img, power)
        else:
            ctx.env_upload(self.np_img, power)
