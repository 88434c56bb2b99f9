"""ctypes binding of include/vplines_frontend.h (EDLines extractor + KLT line matcher on the GPU)."""
import ctypes as C
import os

import numpy as np

from .capi import load_hip_library


class EdlineParam(C.Structure):
    _fields_ = [("ksize", C.c_int), ("sigma", C.c_float), ("gradientThreshold", C.c_float),
                ("anchorThreshold", C.c_float), ("scanIntervals", C.c_int), ("minLineLen", C.c_int),
                ("lineFitErrThreshold", C.c_double)]


class Line(C.Structure):
    _fields_ = [("line_endpoint", C.c_float * 4), ("line_equation", C.c_double * 3), ("center", C.c_float * 2),
                ("length", C.c_float)]


class MatchParam(C.Structure):
    _fields_ = [("step", C.c_int), ("closest_line_threshold", C.c_float), ("line_matching_ratio", C.c_float),
                ("line_distance_error_ratio", C.c_float), ("klt_error_threshold", C.c_float),
                ("illumination_adapt", C.c_int), ("topological_filter", C.c_int),
                ("topo_distance_threshold", C.c_float), ("topo_length_tolerate_ratio", C.c_float),
                ("topo_violation_ratio", C.c_float)]


def default_match_param(illumination_adapt=True, topological_filter=True):
    """LineMatching() defaults (line_matching.h:14-18,45-47) with the tracker's flags (line_feature_tracker.cpp:307-308)"""
    return MatchParam(10, 0.5, 0.4, 3.0, 40.0, int(illumination_adapt), int(topological_filter), 15.0, 0.2, 0.05)


class TrackerOptions(C.Structure):
    """vpl_trk_options"""
    _fields_ = [("ed", EdlineParam), ("match", MatchParam), ("max_h_lines", C.c_int), ("max_v_lines", C.c_int),
                ("equalize", C.c_int), ("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float)]


class TrackerResult(C.Structure):
    """vpl_trk_result"""
    _fields_ = [("n_detected", C.c_int), ("n_lines", C.c_int), ("lines_exist", C.c_int), ("matched", C.c_int),
                ("n_tracked", C.c_int), ("vp_ran", C.c_int), ("vp_status", C.c_int), ("vps", C.c_double * 9),
                ("allfeature_cnt", C.c_int)]


class PointCamera(C.Structure):
    """vpl_pt_camera: PinholeCamera with radial-tangential distortion"""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]


class PointTrackerOptions(C.Structure):
    """vpl_ptrk_options"""
    _fields_ = [("max_cnt", C.c_int), ("min_dist", C.c_int), ("f_threshold", C.c_double), ("focal_length", C.c_double),
                ("equalize", C.c_int), ("clip_limit", C.c_double), ("tiles_x", C.c_int), ("tiles_y", C.c_int)] + \
               [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]


class PointTrackerResult(C.Structure):
    """vpl_ptrk_result: counts after each stage"""
    _fields_ = [(k, C.c_int) for k in ("tracked", "after_border", "after_f", "after_mask", "detected", "published")]


# numpy view of vpl_line (56 bytes) for bulk packing / unpacking without per-line Python loops
LINE_DTYPE = np.dtype({"names": ["line_endpoint", "line_equation", "center", "length"],
                       "formats": [("<f4", 4), ("<f8", 3), ("<f4", 2), "<f4"],
                       "offsets": [0, 16, 40, 48], "itemsize": 56})
assert LINE_DTYPE.itemsize == C.sizeof(Line)


def lines_to_records(a, out):
    """[n,10] doubles (x1,y1,x2,y2,eq0..2,cx,cy,len) -> out[:n] (LINE_DTYPE records)"""
    n = len(a)
    if n:
        a = np.asarray(a, np.float64)
        out["line_endpoint"][:n] = a[:, 0:4]
        out["line_equation"][:n] = a[:, 4:7]
        out["center"][:n] = a[:, 7:9]
        out["length"][:n] = a[:, 9]


def records_to_lines(rec):
    out = np.empty((len(rec), 10))
    out[:, 0:4] = rec["line_endpoint"]
    out[:, 4:7] = rec["line_equation"]
    out[:, 7:9] = rec["center"]
    out[:, 9] = rec["length"]
    return out


BLUR_NORMALISED, BLUR_OPENCV_341 = 0, 1
LINE_FILTER_PARALLEL_DEFAULT = 0.0348994967   # sin(3 degrees), line_matching.h:37


def default_param():
    """production values: line_feature_tracker_node.cpp:203 / config/euroc/euroc_config.yaml:84-87"""
    p = EdlineParam()
    p.ksize, p.sigma, p.gradientThreshold, p.anchorThreshold = 5, 1.0, 30.0, 5.0
    p.scanIntervals, p.minLineLen, p.lineFitErrThreshold = 2, 35, 1.8
    return p


_bound = False


def _bind(lib):
    global _bound
    if _bound:
        return
    vp = C.c_void_p
    lib.vpl_edline_default_param.argtypes = [C.POINTER(EdlineParam)]
    lib.vpl_fe_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vpl_fe_destroy.argtypes = [vp]
    lib.vpl_fe_destroy.restype = None
    lib.vpl_fe_set_stream.argtypes = [vp, vp]
    lib.vpl_fe_synchronize.argtypes = [vp]
    lib.vpl_fe_last_error.argtypes = [vp]
    lib.vpl_fe_last_error.restype = C.c_char_p
    lib.vpl_edlines_upload.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8)]
    lib.vpl_vp_detect_batch.argtypes = [vp, C.c_int, C.POINTER(Line), C.POINTER(C.c_int), C.POINTER(Line), C.POINTER(C.c_int),
                                        C.c_float, C.c_float, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                        C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.vpl_vp_debug.argtypes = [vp, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.vpl_pre_set_maps.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.vpl_pre_upload.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8)]
    lib.vpl_pre_run.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int]
    lib.vpl_pre_download.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8)]
    lib.vpl_pre_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    lib.vpl_edlines_detect.argtypes = [vp, C.POINTER(EdlineParam)]
    lib.vpl_edlines_detect_ex.argtypes = [vp, C.POINTER(EdlineParam), C.c_int]
    lib.vpl_edlines_detect_batch_ex.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(EdlineParam), C.c_int,
                                                C.POINTER(Line), C.POINTER(C.c_int)]
    lib.vpl_fe_set_blur_kernel.argtypes = [vp, C.c_int]
    lib.vpl_fe_keep_blurred.argtypes = [vp, C.c_int]
    lib.vpl_edlines_debug_blurred.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8)]
    lib.vpl_line_filter_detected.argtypes = [vp, C.c_float, C.c_float]
    lib.vpl_line_filter_batch.argtypes = [vp, C.c_int, C.POINTER(Line), C.POINTER(C.c_int), C.c_float, C.c_float]
    lib.vpl_edlines_download.argtypes = [vp, C.c_int, C.POINTER(Line), C.POINTER(C.c_int)]
    lib.vpl_edlines_detect_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(EdlineParam), C.POINTER(Line),
                                             C.POINTER(C.c_int)]
    lib.vpl_edlines_debug_stage.argtypes = [vp, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(C.c_int)] + [C.c_void_p] * 3 + \
                                           [C.POINTER(C.c_int)]
    ip = C.POINTER(C.c_int)
    lib.vpl_edlines_debug_route_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_ulonglong)]
    lib.vpl_match_default_param.argtypes = [C.POINTER(MatchParam)]
    lib.vpl_match_reserve.argtypes = [vp, C.c_int, C.c_int]
    lib.vpl_match_upload.argtypes = [vp, C.c_int, ip, ip, C.POINTER(Line), ip, C.POINTER(Line), ip]
    lib.vpl_match_run.argtypes = [vp, C.POINTER(MatchParam)]
    lib.vpl_match_from_detected.argtypes = [vp, C.c_int, ip, ip, C.c_int]
    lib.vpl_match_counts.argtypes = [vp, C.c_int, ip, ip]
    lib.vpl_match_download.argtypes = [vp, C.c_int, ip, ip]
    lib.vpl_line_match_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.c_int, ip, ip, C.POINTER(Line), ip,
                                         C.POINTER(Line), ip, C.POINTER(MatchParam), ip, ip]
    lib.vpl_match_debug_kps.argtypes = [vp, C.c_int, C.c_int] + [C.c_void_p] * 5 + [ip]
    lib.vpl_match_debug_level.argtypes = [vp, C.c_int, C.c_int, C.c_void_p, C.c_void_p, ip, ip]
    lib.vpl_fe_enable_kernel_timing.argtypes = [vp, C.c_int]
    lib.vpl_fe_kernel_times.argtypes = [vp, ip, C.POINTER(C.c_char_p), C.POINTER(C.c_double)]
    fp = C.POINTER(C.c_float)
    lib.vpl_trk_default_options.argtypes = [C.POINTER(TrackerOptions)]
    lib.vpl_trk_default_options.restype = None
    lib.vpl_trk_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.POINTER(TrackerOptions)]
    lib.vpl_trk_destroy.argtypes = [vp]
    lib.vpl_trk_destroy.restype = None
    lib.vpl_trk_reset.argtypes = [vp, C.c_int]
    lib.vpl_trk_frame.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(TrackerResult), ip, C.POINTER(C.c_double)]
    lib.vpl_trk_get_frame.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(Line), ip, ip, ip, ip, ip]
    lib.vpl_trk_debug_ids.argtypes = [vp, C.c_int, fp, C.c_int, ip, ip, C.c_int, ip, C.c_int, C.c_int, ip, ip, ip, ip, ip, ip]
    lib.vpl_fe_debug_allocs.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    dp = C.POINTER(C.c_double)
    lib.vpl_pt_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.vpl_ptrk_default_options.argtypes = [C.POINTER(PointTrackerOptions)]
    lib.vpl_ptrk_default_options.restype = None
    lib.vpl_ptrk_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.POINTER(PointTrackerOptions)]
    lib.vpl_ptrk_destroy.argtypes = [vp]
    lib.vpl_ptrk_destroy.restype = None
    lib.vpl_ptrk_set_mask.argtypes = [vp, C.POINTER(C.c_uint8)]
    lib.vpl_ptrk_reset.argtypes = [vp, C.c_int]
    lib.vpl_ptrk_frame.argtypes = [vp, C.POINTER(C.c_uint8), dp, ip, C.POINTER(C.c_ulonglong), C.POINTER(PointTrackerResult), ip, dp]
    lib.vpl_ptrk_get_frame.argtypes = [vp, C.c_int, ip, fp, ip, ip, fp, fp, fp, ip]
    lib.vpl_pt_flow_batch.argtypes = [vp, C.c_int, ip, ip, fp, ip, fp, C.POINTER(C.c_uint8)]
    lib.vpl_pt_reject_f_batch.argtypes = [vp, C.c_int, fp, fp, ip, C.POINTER(PointCamera), C.c_double, C.c_double,
                                          C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint8)]
    lib.vpl_pt_detect_batch.argtypes = [vp, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), ip, ip, dp, fp, fp, ip]
    lib.vpl_pt_debug_detect.argtypes = [vp, C.c_int, fp, ip]
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_ulonglong)
    lib.vpl_lc_reserve.argtypes = [vp, C.c_int, C.c_int]
    lib.vpl_lc_set_pattern.argtypes = [vp, C.c_int, ip, ip, ip, ip]
    lib.vpl_lc_keyframe_batch.argtypes = [vp, C.c_int, u8p, fp, ip, C.POINTER(PointCamera), C.c_int, fp, fp, ip, u64p, u64p]
    lib.vpl_lc_debug_frame.argtypes = [vp, C.c_int, u8p, u8p]
    lib.vpl_lc_match_batch.argtypes = [vp, C.c_int, u64p, ip, u64p, fp, fp, ip, fp, fp, u8p, ip, ip]
    _bound = True


class FrontendContext:
    def __init__(self, device=0, max_images=1, width=752, height=480, max_lines=1024, stream=None):
        self.lib = load_hip_library()
        _bind(self.lib)
        self.h = C.c_void_p()
        self.W, self.H, self.max_lines, self.max_images = width, height, max_lines, max_images
        rc = self.lib.vpl_fe_create(C.byref(self.h), device, max_images, width, height, max_lines)
        if rc != 0:
            raise RuntimeError("vpl_fe_create failed: %d (no HIP device? there is no CPU fallback)" % rc)
        if stream is not None:
            self._check(self.lib.vpl_fe_set_stream(self.h, C.c_void_p(stream)), "vpl_fe_set_stream")
        self.n = 0

    def debug_guards(self):
        """VPL_DEBUG_GUARDS=1 (set before the context is made): number of device arrays with a write behind their end"""
        return int(self.lib.vpl_fe_debug_guards(self.h))

    def debug_allocs(self):
        """(arrays in the context's allocation record, their payload bytes): the context's own, the lazily made ones included,
        and those of the tracker session it lends itself to"""
        n, b = C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.vpl_fe_debug_allocs(self.h, C.byref(n), C.byref(b)), "vpl_fe_debug_allocs")
        return int(n.value), int(b.value)

    def close(self):
        if self.h and getattr(self, "_trk", None) is not None:
            self._trk.close()                      # the session goes before the context it borrows
        if self.h and getattr(self, "_ptrk", None) is not None:
            self._ptrk.close()
        if self.h and getattr(self, "_ld", None) is not None:
            self._ld.close()
        if self.h:
            bad = self.debug_guards() if os.environ.get("VPL_DEBUG_GUARDS") == "1" else 0
            msg = self.lib.vpl_fe_last_error(self.h).decode() if bad else ""
            self.lib.vpl_fe_destroy(self.h)
            self.h = C.c_void_p()
            if bad:
                import sys
                print("vpl_fe_debug_guards: %d arrays overrun; %s" % (bad, msg), file=sys.stderr)    # (also when closed by __del__)
                raise RuntimeError("vpl_fe_debug_guards: %d arrays overrun; %s" % (bad, msg))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.lib.vpl_fe_last_error(self.h).decode()))

    def upload(self, images):
        images = np.ascontiguousarray(images, np.uint8)
        assert images.ndim == 3 and images.shape[1:] == (self.H, self.W)
        self.n = images.shape[0]
        self._img = images
        self._check(self.lib.vpl_edlines_upload(self.h, self.n, images.ctypes.data_as(C.POINTER(C.c_uint8))), "upload")

    # ---- image preparation (remap + CLAHE), line_feature_tracker.cpp:62-68 ----
    def set_maps(self, map_x, map_y):
        """float32 [H][W] undistortion maps; None, None switches the remap off"""
        fp = C.POINTER(C.c_float)
        if map_x is None:
            self._check(self.lib.vpl_pre_set_maps(self.h, None, None), "vpl_pre_set_maps")
            return
        mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
        assert mx.shape == (self.H, self.W) and my.shape == (self.H, self.W)
        self._check(self.lib.vpl_pre_set_maps(self.h, mx.ctypes.data_as(fp), my.ctypes.data_as(fp)), "vpl_pre_set_maps")

    def pre_upload(self, raw):
        raw = np.ascontiguousarray(raw, np.uint8)
        assert raw.ndim == 3 and raw.shape[1:] == (self.H, self.W)
        self.n = raw.shape[0]
        self._img = raw
        self._check(self.lib.vpl_pre_upload(self.h, self.n, raw.ctypes.data_as(C.POINTER(C.c_uint8))), "vpl_pre_upload")

    def pre_run(self, equalize=True, clip_limit=3.0, tiles=(8, 8)):
        self._check(self.lib.vpl_pre_run(self.h, int(equalize), clip_limit, tiles[0], tiles[1]), "vpl_pre_run")

    def pre_download(self):
        out = np.empty((self.n, self.H, self.W), np.uint8)
        self._check(self.lib.vpl_pre_download(self.h, self.n, out.ctypes.data_as(C.POINTER(C.c_uint8))), "vpl_pre_download")
        return out

    # ---- vanishing points (vanishing_point_detection.cpp) ----
    def vp_detect(self, hyp_lines, all_lines, f, cx, cy, seeds, first_frame):
        """hyp_lines / all_lines: per frame an [k][>=4] array whose first 4 columns are the end points.
        Returns vps [n][3][3], ids (list of int arrays), status [n]."""
        n = len(hyp_lines)
        ML = self.max_lines

        def pack(lists):
            rec = np.zeros(n * ML, LINE_DTYPE)
            cnt = np.zeros(n, np.int32)
            for i, l in enumerate(lists):
                l = np.asarray(l, np.float64).reshape(-1, np.asarray(l).shape[-1] if len(l) else 4)
                cnt[i] = len(l)
                rec["line_endpoint"][i * ML:i * ML + len(l)] = l[:, :4]
            return rec, cnt
        rh, nh = pack(hyp_lines)
        ra, na = pack(all_lines)
        seeds = np.ascontiguousarray(seeds, np.uint32)
        first = np.ascontiguousarray(first_frame, np.int32)
        vps = np.zeros((n, 3, 3))
        ids = np.zeros((n, ML), np.int32)
        status = np.zeros(n, np.int32)
        ip = C.POINTER(C.c_int)
        self._check(self.lib.vpl_vp_detect_batch(self.h, n, rh.ctypes.data_as(C.POINTER(Line)), nh.ctypes.data_as(ip),
                                                 ra.ctypes.data_as(C.POINTER(Line)), na.ctypes.data_as(ip), f, cx, cy,
                                                 seeds.ctypes.data_as(C.POINTER(C.c_uint32)), first.ctypes.data_as(ip),
                                                 vps.ctypes.data_as(C.POINTER(C.c_double)), ids.ctypes.data_as(ip),
                                                 status.ctypes.data_as(ip)), "vpl_vp_detect_batch")
        return vps, [ids[i, :na[i]].copy() for i in range(n)], status

    def vp_debug(self, frame):
        grid = np.zeros((90, 360))
        pairs = np.zeros((105, 2), np.int32)
        best, drawn = C.c_int(), C.c_int()
        self._check(self.lib.vpl_vp_debug(self.h, frame, grid.ctypes.data, pairs.ctypes.data, C.byref(best), C.byref(drawn)),
                    "vpl_vp_debug")
        return grid, pairs, best.value, drawn.value

    def detect(self, param=None, smoothed=True):
        """EDline(image, lines, smoothed) for the uploaded batch; smoothed=False (the reference's default) runs the Gaussian
        pre-blur of EdgeDrawing first (edline_detector.cpp:82-84)"""
        self._param = param or default_param()
        self._check(self.lib.vpl_edlines_detect_ex(self.h, C.byref(self._param), 1 if smoothed else 0), "vpl_edlines_detect_ex")

    def set_blur_kernel(self, mode):
        """BLUR_NORMALISED (default, OpenCV 3.4.9+ / 4.2+) or BLUR_OPENCV_341"""
        self._check(self.lib.vpl_fe_set_blur_kernel(self.h, int(mode)), "vpl_fe_set_blur_kernel")

    def keep_blurred(self, on=True):
        self._check(self.lib.vpl_fe_keep_blurred(self.h, 1 if on else 0), "vpl_fe_keep_blurred")

    def debug_blurred(self, img):
        out = np.empty((self.H, self.W), np.uint8)
        self._check(self.lib.vpl_edlines_debug_blurred(self.h, img, out.ctypes.data_as(C.POINTER(C.c_uint8))),
                    "vpl_edlines_debug_blurred")
        return out

    def line_filter_detected(self, distance_threshold, parallel_threshold=LINE_FILTER_PARALLEL_DEFAULT):
        """LineMatching::LineFilter (line_matching.cpp:167-264) on the lines of the last detect, in HBM"""
        self._check(self.lib.vpl_line_filter_detected(self.h, distance_threshold, parallel_threshold), "vpl_line_filter_detected")

    def line_filter_batch(self, lines, distance_threshold, parallel_threshold=LINE_FILTER_PARALLEL_DEFAULT):
        """LineFilter on caller-owned lists: lines = list of [k,10] arrays; returns the filtered lists"""
        n, ML = len(lines), self.max_lines
        rec = np.zeros(n * ML, LINE_DTYPE)
        cnt = np.zeros(n, np.int32)
        for i, l in enumerate(lines):
            cnt[i] = len(l)
            lines_to_records(l, rec[i * ML:i * ML + len(l)])
        self._check(self.lib.vpl_line_filter_batch(self.h, n, rec.ctypes.data_as(C.POINTER(Line)),
                                                   cnt.ctypes.data_as(C.POINTER(C.c_int)), distance_threshold,
                                                   parallel_threshold), "vpl_line_filter_batch")
        return [records_to_lines(rec[i * ML:i * ML + cnt[i]]) for i in range(n)]

    def enable_kernel_timing(self, on=True):
        self._check(self.lib.vpl_fe_enable_kernel_timing(self.h, 1 if on else 0), "vpl_fe_enable_kernel_timing")

    def kernel_times(self):
        """{kernel: total ms} of the launches since timing was enabled (hipEvents on the context's stream)"""
        cnt = C.c_int(256)
        names = (C.c_char_p * 256)()
        ms = (C.c_double * 256)()
        self._check(self.lib.vpl_fe_kernel_times(self.h, C.byref(cnt), names, ms), "vpl_fe_kernel_times")
        out = {}
        for i in range(cnt.value):
            out[names[i].decode()] = out.get(names[i].decode(), 0.0) + ms[i]
        return out

    def synchronize(self):
        self._check(self.lib.vpl_fe_synchronize(self.h), "vpl_fe_synchronize")

    def download(self):
        rec = np.zeros(self.n * self.max_lines, LINE_DTYPE)
        counts = (C.c_int * self.n)()
        self._check(self.lib.vpl_edlines_download(self.h, self.n, rec.ctypes.data_as(C.POINTER(Line)), counts),
                    "vpl_edlines_download")
        return [records_to_lines(rec[i * self.max_lines:i * self.max_lines + counts[i]]) for i in range(self.n)]

    def detect_batch(self, images, param=None, smoothed=True):
        self.upload(images)
        self.detect(param, smoothed)
        self.synchronize()
        return self.download()

    def debug_stage(self, img):
        W, H = self.W, self.H
        N = W * H
        cap = N // 5
        dx = np.zeros(N, np.int16); dy = np.zeros(N, np.int16); g = np.zeros(N, np.int16); d = np.zeros(N, np.uint8)
        anchors = np.zeros((cap, 2), np.uint32); nA = C.c_int(0)
        cx = np.zeros(2 * cap, np.uint32); cy = np.zeros(2 * cap, np.uint32); sid = np.zeros(cap // 20 + 2, np.uint32)
        nE = C.c_int(0)
        p = lambda a: C.c_void_p(a.ctypes.data)
        self._check(self.lib.vpl_edlines_debug_stage(self.h, img, p(dx), p(dy), p(g), p(d), p(anchors), C.byref(nA), p(cx),
                                                     p(cy), p(sid), C.byref(nE)), "vpl_edlines_debug_stage")
        ne = nE.value
        npx = int(sid[ne])
        return dict(dx=dx.reshape(H, W), dy=dy.reshape(H, W), g=g.reshape(H, W), dir=d.reshape(H, W),
                    anchors=anchors[:nA.value], chain_x=cx[:npx], chain_y=cy[:npx], sid=sid[:ne + 1])

    def route_stats(self, img):
        out = (C.c_ulonglong * 4)()
        self._check(self.lib.vpl_edlines_debug_route_stats(self.h, img, out), "vpl_edlines_debug_route_stats")
        return dict(steps=out[0], tile_loads=out[1], walks=out[2], cycles=out[3])

    # ---- KLT line matching ---------------------------------------------------------------------------------
    def match_reserve(self, max_pairs, max_kps=4096):
        self.max_pairs, self.max_kps = max_pairs, max_kps
        self._check(self.lib.vpl_match_reserve(self.h, max_pairs, max_kps), "vpl_match_reserve")

    def _pack_lines(self, per_pair):
        rec = np.zeros(len(per_pair) * self.max_lines, LINE_DTYPE)
        cnt = (C.c_int * len(per_pair))()
        for i, L in enumerate(per_pair):
            cnt[i] = len(L)
            if len(L) <= self.max_lines:   # otherwise the library reports VPL_E_CAPACITY
                lines_to_records(L, rec[i * self.max_lines:(i + 1) * self.max_lines])
        return rec, cnt

    def match_upload(self, pairs, lines_ref, lines_cur):
        """pairs: list of (ref image index, cur image index); lines_*: per pair [n,10] arrays"""
        self.n_pairs = len(pairs)
        ri = (C.c_int * self.n_pairs)(*[p[0] for p in pairs])
        ci = (C.c_int * self.n_pairs)(*[p[1] for p in pairs])
        lr, nr = self._pack_lines(lines_ref)
        lc, nc = self._pack_lines(lines_cur)
        self._nref = [len(L) for L in lines_ref]
        self._check(self.lib.vpl_match_upload(self.h, self.n_pairs, ri, ci, lr.ctypes.data_as(C.POINTER(Line)), nr,
                                              lc.ctypes.data_as(C.POINTER(Line)), nc), "vpl_match_upload")

    def match_from_detected(self, pairs, max_lines=None):
        """vpl_match_from_detected: the lines of the last detect() as the matcher's input, device to device"""
        self.n_pairs = len(pairs)
        ri = (C.c_int * self.n_pairs)(*[p[0] for p in pairs])
        ci = (C.c_int * self.n_pairs)(*[p[1] for p in pairs])
        self._check(self.lib.vpl_match_from_detected(self.h, self.n_pairs, ri, ci, int(max_lines or self.max_lines)),
                    "vpl_match_from_detected")
        self._nref = None

    def match_counts(self):
        nr, nc = (C.c_int * self.n_pairs)(), (C.c_int * self.n_pairs)()
        self._check(self.lib.vpl_match_counts(self.h, self.n_pairs, nr, nc), "vpl_match_counts")
        return [int(x) for x in nr], [int(x) for x in nc]

    def match_run(self, param=None):
        self._mparam = param or default_match_param()
        self._check(self.lib.vpl_match_run(self.h, C.byref(self._mparam)), "vpl_match_run")

    def match_download(self):
        a = np.full((self.n_pairs, self.max_lines), -2, np.int32)
        ok = (C.c_int * self.n_pairs)()
        self._check(self.lib.vpl_match_download(self.h, self.n_pairs, a.ctypes.data_as(C.POINTER(C.c_int)), ok),
                    "vpl_match_download")
        if self._nref is None:
            self._nref = self.match_counts()[0]
        return [a[i, :self._nref[i]].copy() for i in range(self.n_pairs)], [int(x) for x in ok]

    def match_batch(self, images, pairs, lines_ref, lines_cur, param=None):
        self.upload(images)
        self.match_upload(pairs, lines_ref, lines_cur)
        self.match_run(param)
        self.synchronize()
        return self.match_download()

    def match_debug_kps(self, pair):
        cap = self.max_kps
        kr = np.zeros((cap, 2), np.float32); kc = np.zeros((cap, 2), np.float32)
        st = np.zeros(cap, np.uint8); er = np.zeros(cap, np.float32); k2l = np.zeros(cap, np.int32)
        nk = C.c_int(0)
        p = lambda a: C.c_void_p(a.ctypes.data)
        self._check(self.lib.vpl_match_debug_kps(self.h, pair, cap, p(kr), p(kc), p(st), p(er), p(k2l), C.byref(nk)),
                    "vpl_match_debug_kps")
        n = nk.value
        return dict(kps_ref=kr[:n], kps_cur=kc[:n], status=st[:n], err=er[:n], kp2line_cur=k2l[:n])

    def match_debug_level(self, img, level):
        w, h = C.c_int(0), C.c_int(0)
        self._check(self.lib.vpl_match_debug_level(self.h, img, level, None, None, C.byref(w), C.byref(h)),
                    "vpl_match_debug_level")
        px = np.zeros((h.value, w.value), np.uint8); d = np.zeros((h.value, w.value, 2), np.int16)
        self._check(self.lib.vpl_match_debug_level(self.h, img, level, C.c_void_p(px.ctypes.data),
                                                   C.c_void_p(d.ctypes.data), C.byref(w), C.byref(h)),
                    "vpl_match_debug_level")
        return px, d

    # ---- point front-end: goodFeaturesToTrack (cvmodified.cpp:38-216) ---------------------------------------
    def pt_reserve(self, max_candidates=8192, max_corners=256, max_points=256):
        self.pt_max_candidates, self.pt_max_corners, self.pt_max_points = max_candidates, max_corners, max_points
        self._check(self.lib.vpl_pt_reserve(self.h, max_candidates, max_corners, max_points), "vpl_pt_reserve")

    def _pack_points(self, lists):
        n, MP = len(lists), self.pt_max_points
        a = np.zeros((n, MP, 2), np.float32)
        cnt = np.zeros(n, np.int32)
        for i, l in enumerate(lists):
            l = np.asarray(l, np.float32).reshape(-1, 2)
            cnt[i] = len(l)
            if len(l) <= MP:               # otherwise the library reports VPL_E_CAPACITY
                a[i, :len(l)] = l
        return a, cnt

    def pt_flow(self, pairs, prev_pts):
        """calcOpticalFlowPyrLK(21 x 21, 3 levels) on the frames in the context's slots (upload() / pre_run()): pairs a list of
        (prev image, next image), prev_pts per pair a [k][2] array.  Returns per pair (next_pts [k][2] float32, status [k] uint8)."""
        n = len(pairs)
        pi = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        ni = np.ascontiguousarray([p[1] for p in pairs], np.int32)
        prev, cnt = self._pack_points(prev_pts)
        assert len(cnt) == n
        nxt = np.zeros_like(prev)
        status = np.zeros((n, self.pt_max_points), np.uint8)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self._check(self.lib.vpl_pt_flow_batch(self.h, n, pi.ctypes.data_as(ip), ni.ctypes.data_as(ip), prev.ctypes.data_as(fp),
                                               cnt.ctypes.data_as(ip), nxt.ctypes.data_as(fp), status.ctypes.data_as(C.POINTER(C.c_uint8))),
                    "vpl_pt_flow_batch")
        return [(nxt[i, :cnt[i]].copy(), status[i, :cnt[i]].copy()) for i in range(n)]

    def pt_reject_f(self, cur_pts, forw_pts, camera, seeds, focal_length=460.0, f_threshold=1.0):
        """rejectWithF for a batch: cur_pts / forw_pts lists of [k][2] arrays, camera a PointCamera, seeds one per list.
        Returns per list the 0 / 1 status [k] (uint8)."""
        cur, cnt = self._pack_points(cur_pts)
        forw, cnt2 = self._pack_points(forw_pts)
        assert np.array_equal(cnt, cnt2)
        n = len(cnt)
        seeds = np.ascontiguousarray(seeds, np.uint64)
        assert seeds.shape == (n,)
        status = np.zeros((n, self.pt_max_points), np.uint8)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self._check(self.lib.vpl_pt_reject_f_batch(self.h, n, cur.ctypes.data_as(fp), forw.ctypes.data_as(fp), cnt.ctypes.data_as(ip),
                                                   C.byref(camera), focal_length, f_threshold,
                                                   seeds.ctypes.data_as(C.POINTER(C.c_ulonglong)), status.ctypes.data_as(C.POINTER(C.c_uint8))),
                    "vpl_pt_reject_f_batch")
        return [status[i, :cnt[i]].copy() for i in range(n)]

    def pt_detect(self, images, max_corners, min_distance, masks=None):
        """images [n][H][W] uint8 (None: the frames in the context's slots, n = len(max_corners)); max_corners, min_distance:
        a number or one per image; masks: None, or a list with per image an [H][W] plane (non-zero = allowed) or None.
        Returns per image (corners [k][2] float32, scores [k] float32)."""
        u8 = C.POINTER(C.c_uint8)
        if images is not None:
            images = np.ascontiguousarray(images, np.uint8)
            assert images.ndim == 3 and images.shape[1:] == (self.H, self.W)
            n = images.shape[0]
            self.n = n
        else:
            n = len(max_corners)
        mc = np.ascontiguousarray(np.broadcast_to(np.asarray(max_corners, np.int32), (n,)))
        md = np.ascontiguousarray(np.broadcast_to(np.asarray(min_distance, np.float64), (n,)))
        mp, up = None, None
        if masks is not None and any(m is not None for m in masks):
            assert len(masks) == n
            planes = np.zeros((n, self.H, self.W), np.uint8)
            use = np.zeros(n, np.int32)
            for i, m in enumerate(masks):
                if m is not None:
                    planes[i] = np.asarray(m, np.uint8)
                    use[i] = 1
            mp, up = planes.ctypes.data_as(u8), use.ctypes.data_as(C.POINTER(C.c_int))
        MC = self.pt_max_corners
        corners = np.zeros((n, MC, 2), np.float32)
        scores = np.zeros((n, MC), np.float32)
        counts = np.zeros(n, np.int32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self._check(self.lib.vpl_pt_detect_batch(self.h, n, images.ctypes.data_as(u8) if images is not None else None, mp, up,
                                                 mc.ctypes.data_as(ip), md.ctypes.data_as(C.POINTER(C.c_double)),
                                                 corners.ctypes.data_as(fp), scores.ctypes.data_as(fp), counts.ctypes.data_as(ip)),
                    "vpl_pt_detect_batch")
        return [(corners[i, :counts[i]].copy(), scores[i, :counts[i]].copy()) for i in range(n)]

    def pt_debug_detect(self, img):
        """test access: (cornerMinEigenVal plane [H][W] float32, candidates found) of frame `img` of the last pt_detect"""
        eig = np.zeros((self.H, self.W), np.float32)
        nc = C.c_int(0)
        self._check(self.lib.vpl_pt_debug_detect(self.h, img, eig.ctypes.data_as(C.POINTER(C.c_float)), C.byref(nc)),
                    "vpl_pt_debug_detect")
        return eig, nc.value

    # ---- loop-closure front-end: KeyFrame's FAST / BRIEF and searchByBRIEFDes (pose_graph/src/keyframe.cpp) ----
    def lc_reserve(self, max_keypoints=8192, max_window_points=256):
        self.lc_max_keypoints, self.lc_max_window_points = max_keypoints, max_window_points
        self._check(self.lib.vpl_lc_reserve(self.h, max_keypoints, max_window_points), "vpl_lc_reserve")

    def lc_set_pattern(self, x1, y1, x2, y2):
        """the BRIEF test pairs (brief_pattern.yml of the reference): four lists of 256 integers"""
        p = [np.ascontiguousarray(a, np.int32) for a in (x1, y1, x2, y2)]
        assert all(a.shape == p[0].shape and a.ndim == 1 for a in p)
        ip = C.POINTER(C.c_int)
        self._check(self.lib.vpl_lc_set_pattern(self.h, len(p[0]), *[a.ctypes.data_as(ip) for a in p]), "vpl_lc_set_pattern")

    def lc_keyframe(self, images, window_pts, camera, fast_threshold=20, out=None):
        """images [n][H][W] uint8 (None: the frames in the context's slots, n = len(window_pts)); window_pts per frame a [k][2]
        array of pixel positions; camera a PointCamera.  Returns per frame a dict: keypoints [m][2], keypoints_norm [m][2] float32,
        brief [m][4] uint64, window_brief [k][4] uint64.  out (tests): the raw output arrays to write into."""
        u8 = C.POINTER(C.c_uint8)
        if images is not None:
            images = np.ascontiguousarray(images, np.uint8)
            assert images.ndim == 3 and images.shape[1:] == (self.H, self.W)
            assert len(window_pts) == images.shape[0]
            self.n = images.shape[0]
        n, KP, WP = len(window_pts), self.lc_max_keypoints, self.lc_max_window_points
        win = np.zeros((n, WP, 2), np.float32)
        wcnt = np.zeros(n, np.int32)
        for i, l in enumerate(window_pts):
            l = np.asarray(l, np.float32).reshape(-1, 2)
            wcnt[i] = len(l)
            if len(l) <= WP:               # otherwise the library reports VPL_E_CAPACITY
                win[i, :len(l)] = l
        if out is None:
            out = (np.zeros((n, KP, 2), np.float32), np.zeros((n, KP, 2), np.float32), np.zeros(n, np.int32),
                   np.zeros((n, KP, 4), np.uint64), np.zeros((n, WP, 4), np.uint64))
        kp, kn, cnt, br, wbr = out
        ip, fp, u64 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)
        self._check(self.lib.vpl_lc_keyframe_batch(self.h, n, images.ctypes.data_as(u8) if images is not None else None,
                                                   win.ctypes.data_as(fp), wcnt.ctypes.data_as(ip), C.byref(camera), fast_threshold,
                                                   kp.ctypes.data_as(fp), kn.ctypes.data_as(fp), cnt.ctypes.data_as(ip),
                                                   br.ctypes.data_as(u64), wbr.ctypes.data_as(u64)), "vpl_lc_keyframe_batch")
        return [dict(keypoints=kp[i, :cnt[i]].copy(), keypoints_norm=kn[i, :cnt[i]].copy(), brief=br[i, :cnt[i]].copy(),
                     window_brief=wbr[i, :wcnt[i]].copy()) for i in range(n)]

    def lc_debug_frame(self, img):
        """test access: (blurred plane, FAST score plane) [H][W] uint8 of frame `img` of the last lc_keyframe"""
        b, s = np.zeros((self.H, self.W), np.uint8), np.zeros((self.H, self.W), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._check(self.lib.vpl_lc_debug_frame(self.h, img, b.ctypes.data_as(u8), s.ctypes.data_as(u8)), "vpl_lc_debug_frame")
        return b, s

    def lc_match(self, window_brief, old_brief, old_keypoints, old_keypoints_norm):
        """searchByBRIEFDes for a batch of pairs: per pair the window descriptors [k][4] and the candidate's descriptors [m][4],
        keypoints [m][2] and keypoints_norm [m][2].  Returns per pair a dict: matched_2d_old, matched_2d_old_norm [k][2] float32,
        status [k] uint8, best_dist, best_index [k] int32."""
        n, KP, WP = len(window_brief), self.lc_max_keypoints, self.lc_max_window_points
        assert len(old_brief) == len(old_keypoints) == len(old_keypoints_norm) == n
        wb, ob = np.zeros((n, WP, 4), np.uint64), np.zeros((n, KP, 4), np.uint64)
        okp, onr = np.zeros((n, KP, 2), np.float32), np.zeros((n, KP, 2), np.float32)
        wcnt, ocnt = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for i in range(n):
            w, o = np.asarray(window_brief[i], np.uint64).reshape(-1, 4), np.asarray(old_brief[i], np.uint64).reshape(-1, 4)
            k, q = np.asarray(old_keypoints[i], np.float32).reshape(-1, 2), np.asarray(old_keypoints_norm[i], np.float32).reshape(-1, 2)
            assert len(o) == len(k) == len(q)
            wcnt[i], ocnt[i] = len(w), len(o)
            if len(w) <= WP and len(o) <= KP:   # otherwise the library reports VPL_E_CAPACITY
                wb[i, :len(w)], ob[i, :len(o)], okp[i, :len(o)], onr[i, :len(o)] = w, o, k, q
        m2d, m2n = np.zeros((n, WP, 2), np.float32), np.zeros((n, WP, 2), np.float32)
        st, bd, bi = np.zeros((n, WP), np.uint8), np.zeros((n, WP), np.int32), np.zeros((n, WP), np.int32)
        ip, fp, u64 = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_ulonglong)
        self._check(self.lib.vpl_lc_match_batch(self.h, n, wb.ctypes.data_as(u64), wcnt.ctypes.data_as(ip), ob.ctypes.data_as(u64),
                                                okp.ctypes.data_as(fp), onr.ctypes.data_as(fp), ocnt.ctypes.data_as(ip),
                                                m2d.ctypes.data_as(fp), m2n.ctypes.data_as(fp), st.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                bd.ctypes.data_as(ip), bi.ctypes.data_as(ip)), "vpl_lc_match_batch")
        return [dict(matched_2d_old=m2d[i, :wcnt[i]].copy(), matched_2d_old_norm=m2n[i, :wcnt[i]].copy(), status=st[i, :wcnt[i]].copy(),
                     best_dist=bd[i, :wcnt[i]].copy(), best_index=bi[i, :wcnt[i]].copy()) for i in range(n)]


def reduce_vector(v, status):
    """reduceVector (pose_graph/src/keyframe.cpp:3-11): the entries of v whose status is non-zero, in order"""
    v, status = np.asarray(v), np.asarray(status)
    if len(v) != len(status):
        raise ValueError("reduce_vector: %d entries, %d status flags" % (len(v), len(status)))
    return v[status != 0]


def loop_matches(fe, cur, old):
    """The descriptor step of KeyFrame::findConnection (keyframe.cpp:259-330) for one pair: searchByBRIEFDes of the current
    keyframe's window descriptors against the candidate, then reduceVector of every window list by the match status.
      cur: dict with window_brief [k][4], point_2d_uv [k][2], point_2d_norm [k][2], point_3d [k][3], point_id [k]
      old: dict with brief [m][4], keypoints [m][2], keypoints_norm [m][2] (an entry of FrontendContext.lc_keyframe)
    Returns a dict of the reduced lists: matched_2d_cur, matched_2d_cur_norm, matched_3d, matched_id, matched_2d_old,
    matched_2d_old_norm, and `status`, the unreduced match status."""
    k = len(cur["window_brief"])
    for name in ("point_2d_uv", "point_2d_norm", "point_3d", "point_id"):
        if len(cur[name]) != k:
            raise ValueError("loop_matches: %s has %d entries, window_brief %d" % (name, len(cur[name]), k))
    m = fe.lc_match([cur["window_brief"]], [old["brief"]], [old["keypoints"]], [old["keypoints_norm"]])[0]
    st = m["status"]
    return dict(matched_2d_cur=reduce_vector(cur["point_2d_uv"], st), matched_2d_cur_norm=reduce_vector(cur["point_2d_norm"], st),
                matched_3d=reduce_vector(cur["point_3d"], st), matched_id=reduce_vector(cur["point_id"], st),
                matched_2d_old=reduce_vector(m["matched_2d_old"], st), matched_2d_old_norm=reduce_vector(m["matched_2d_old_norm"], st),
                status=st)


MATCHED_LISTS = ("matched_2d_cur", "matched_2d_cur_norm", "matched_3d", "matched_id", "matched_2d_old", "matched_2d_old_norm")


def find_connection(fe, ctx, cur, old, seed=0, options=None):
    """KeyFrame::findConnection (keyframe.cpp:259-520) for one pair, as the reference chains it: loop_matches (the descriptor
    search and its reduceVector calls) on the front-end context `fe`, then Context.loop_verify on `ctx` (the PnP RANSAC, the
    MIN_LOOP_NUM gates, the relative pose and its acceptance) and, when the PnP ran, the reduceVector calls by its inliers.
      cur: as for loop_matches, and origin_vio_T [3], origin_vio_R [3][3], tic [3], qic [3][3];  seed: of the sample stream
    Returns a dict: has_loop, result (the LoopResult), the six matched lists as findConnection leaves them, match_status [k] and
    pnp_status (None when fewer than min_loop_num + 1 matches were left and nothing ran)."""
    from .capi import LoopInput, LOOP_FEW_POINTS
    m = loop_matches(fe, cur, old)
    q = LoopInput(m["matched_3d"], m["matched_2d_old_norm"], cur["origin_vio_T"], cur["origin_vio_R"], cur["tic"], cur["qic"], seed)
    res, status = ctx.loop_verify([q], options)
    ran = res[0].stage != LOOP_FEW_POINTS
    out = {k: (reduce_vector(m[k], status[0]) if ran else m[k]) for k in MATCHED_LISTS}
    out.update(has_loop=bool(res[0].has_loop), result=res[0], match_status=m["status"], pnp_status=status[0] if ran else None)
    return out


def default_tracker_options(max_h_lines=25, max_v_lines=25, fx=1.0, fy=1.0, cx=0.0, cy=0.0, equalize=True):
    """vpl_trk_default_options with the quota and K_ filled in"""
    lib = load_hip_library()
    _bind(lib)
    o = TrackerOptions()
    lib.vpl_trk_default_options(C.byref(o))
    o.max_h_lines, o.max_v_lines, o.equalize = max_h_lines, max_v_lines, int(equalize)
    o.fx, o.fy, o.cx, o.cy = fx, fy, cx, cy
    return o


class TrackerSession:
    """vpl_trk_*: LineFeatureTracker::readImage for n_seq sequences with the tracker's state resident on the device.
    Borrows a FrontendContext made with max_images >= 2 * n_seq on which match_reserve(>= n_seq, max_kps) was called."""

    def __init__(self, fe, n_seq, options=None):
        self.fe, self.lib, self.n_seq = fe, fe.lib, n_seq
        self.opt = options or default_tracker_options()
        self.h = C.c_void_p()
        fe._check(self.lib.vpl_trk_create(C.byref(self.h), fe.h, n_seq, C.byref(self.opt)), "vpl_trk_create")
        fe._trk = self
        ML = fe.max_lines
        self._res = (TrackerResult * n_seq)()
        self._ids = np.zeros((n_seq, ML), np.int32)
        self._obs = np.zeros((n_seq, ML, 8))

    def close(self):
        if self.h:
            self.lib.vpl_trk_destroy(self.h)
            self.h = C.c_void_p()
            if getattr(self.fe, "_trk", None) is self:
                self.fe._trk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, seq):
        self.fe._check(self.lib.vpl_trk_reset(self.h, seq), "vpl_trk_reset")

    def frame(self, raw, vp_seed):
        """raw [n_seq][H][W] uint8, vp_seed [n_seq] -> per sequence a dict: the fields of vpl_trk_result, `ids` [n_lines] and
        `obs` [n_lines][8] (x1 y1 x2 y2 normalised, vp x y z, vp flag): what vpl_odo_frame takes as line_id / line_obs"""
        raw = np.ascontiguousarray(raw, np.uint8)
        assert raw.shape == (self.n_seq, self.fe.H, self.fe.W)
        seed = np.ascontiguousarray(vp_seed, np.uint32)
        assert seed.shape == (self.n_seq,)
        self.fe._check(self.lib.vpl_trk_frame(self.h, raw.ctypes.data_as(C.POINTER(C.c_uint8)), seed.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              self._res, self._ids.ctypes.data_as(C.POINTER(C.c_int)),
                                              self._obs.ctypes.data_as(C.POINTER(C.c_double))), "vpl_trk_frame")
        out = []
        for s in range(self.n_seq):
            r = self._res[s]
            d = {f: getattr(r, f) for f, _ in TrackerResult._fields_ if f != "vps"}
            d["vps"] = np.array(r.vps).reshape(3, 3)
            d["ids"] = self._ids[s, :r.n_lines].copy()
            d["obs"] = self._obs[s, :r.n_lines].copy()
            out.append(d)
        return out

    def get_frame(self, seq):
        """test access: what curframe_ holds (img, lines records [max_lines], ids, t_cnt) and the last call's match / VP ids"""
        ML, fe = self.fe.max_lines, self.fe
        img = np.zeros((fe.H, fe.W), np.uint8)
        rec = np.zeros(ML, LINE_DTYPE)
        ids, tc, match, vpi = (np.zeros(ML, np.int32) for _ in range(4))
        n_tc = C.c_int(0)
        ip = C.POINTER(C.c_int)
        fe._check(self.lib.vpl_trk_get_frame(self.h, seq, img.ctypes.data_as(C.POINTER(C.c_uint8)), rec.ctypes.data_as(C.POINTER(Line)),
                                             ids.ctypes.data_as(ip), tc.ctypes.data_as(ip), C.byref(n_tc), match.ctypes.data_as(ip),
                                             vpi.ctypes.data_as(ip)), "vpl_trk_get_frame")
        return dict(img=img, lines=rec, ids=ids, t_cnt=tc[:n_tc.value].copy(), match=match, vp_ids=vpi)


def default_point_tracker_options(camera=None, **kw):
    """vpl_ptrk_default_options (150 points, min_dist 30, F threshold 1, focal length 460, CLAHE 3.0 8 x 8) with the camera
    (fx, fy, cx, cy, k1, k2, p1, p2) and any field given by name filled in"""
    lib = load_hip_library()
    _bind(lib)
    o = PointTrackerOptions()
    lib.vpl_ptrk_default_options(C.byref(o))
    if camera is not None:
        o.fx, o.fy, o.cx, o.cy, o.k1, o.k2, o.p1, o.p2 = camera
    for k, val in kw.items():
        setattr(o, k, val)
    return o


class PointTrackerSession:
    """vpl_ptrk_*: FeatureTracker::readImage for n_seq cameras with the tracker's lists resident on the device.  Borrows a
    FrontendContext made with max_images >= 2 * n_seq on which pt_reserve(max_corners, max_points >= max_cnt) was called."""

    def __init__(self, fe, n_seq, options=None):
        self.fe, self.lib, self.n_seq = fe, fe.lib, n_seq
        self.opt = options or default_point_tracker_options()
        self.h = C.c_void_p()
        fe._check(self.lib.vpl_ptrk_create(C.byref(self.h), fe.h, n_seq, C.byref(self.opt)), "vpl_ptrk_create")
        fe._ptrk = self
        MP = fe.pt_max_points
        self._res = (PointTrackerResult * n_seq)()
        self._ids = np.zeros((n_seq, MP), np.int32)
        self._rows = np.zeros((n_seq, MP, 7))

    def close(self):
        if self.h:
            self.lib.vpl_ptrk_destroy(self.h)
            self.h = C.c_void_p()
            if getattr(self.fe, "_ptrk", None) is self:
                self.fe._ptrk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mask(self, plane):
        p = None if plane is None else np.ascontiguousarray(plane, np.uint8)
        assert p is None or p.shape == (self.fe.H, self.fe.W)
        self.fe._check(self.lib.vpl_ptrk_set_mask(self.h, None if p is None else p.ctypes.data_as(C.POINTER(C.c_uint8))), "vpl_ptrk_set_mask")

    def reset(self, seq):
        self.fe._check(self.lib.vpl_ptrk_reset(self.h, seq), "vpl_ptrk_reset")

    def frame(self, raw, time, publish, seed):
        """raw [n_seq][H][W] uint8, time / publish / seed [n_seq] -> per sequence a dict: the fields of vpl_ptrk_result, `ids`
        [published] and `rows` [published][7] (x, y undistorted, u, v, vx, vy, prob): ids and rows[:, :2] with a 1 behind them are
        what vpl_odo_frame takes as pt_id / pt_xy1"""
        raw = np.ascontiguousarray(raw, np.uint8)
        assert raw.shape == (self.n_seq, self.fe.H, self.fe.W)
        tm = np.ascontiguousarray(time, np.float64)
        pub = np.ascontiguousarray(publish, np.int32)
        sd = np.ascontiguousarray(seed, np.uint64)
        assert tm.shape == pub.shape == sd.shape == (self.n_seq,)
        self.fe._check(self.lib.vpl_ptrk_frame(self.h, raw.ctypes.data_as(C.POINTER(C.c_uint8)), tm.ctypes.data_as(C.POINTER(C.c_double)),
                                               pub.ctypes.data_as(C.POINTER(C.c_int)), sd.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                               self._res, self._ids.ctypes.data_as(C.POINTER(C.c_int)),
                                               self._rows.ctypes.data_as(C.POINTER(C.c_double))), "vpl_ptrk_frame")
        out = []
        for s in range(self.n_seq):
            r = self._res[s]
            d = {f: getattr(r, f) for f, _ in PointTrackerResult._fields_}
            d["ids"] = self._ids[s, :r.published].copy()
            d["rows"] = self._rows[s, :r.published].copy()
            out.append(d)
        return out

    def get_frame(self, seq):
        """test access: the tracker's lists after the last accepted call"""
        MP = self.fe.pt_max_points
        n, nid = C.c_int(0), C.c_int(0)
        pts, un = np.zeros((MP, 2), np.float32), np.zeros((MP, 2), np.float32)
        ids, cnt = np.zeros(MP, np.int32), np.zeros(MP, np.int32)
        sc, usc = np.zeros(MP, np.float32), np.zeros(MP, np.float32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        self.fe._check(self.lib.vpl_ptrk_get_frame(self.h, seq, C.byref(n), pts.ctypes.data_as(fp), ids.ctypes.data_as(ip),
                                                   cnt.ctypes.data_as(ip), sc.ctypes.data_as(fp), un.ctypes.data_as(fp),
                                                   usc.ctypes.data_as(fp), C.byref(nid)), "vpl_ptrk_get_frame")
        m = n.value
        return dict(n=m, pts=pts[:m], ids=ids[:m], track_cnt=cnt[:m], scores=sc[:m], un_pts=un[:m], un_scores=usc[:m], next_id=nid.value)


# ---- loop detector: the DBoW2 vocabulary, the keyframe database, PoseGraph::detectLoop (pose_graph/src/pose_graph.cpp:304-386) ----
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3      # DBoW2::WeightingType
L1_NORM = 0                               # DBoW2::ScoringType: the only one taken

VOC_NODE_DTYPE = np.dtype([("node_id", "<i4"), ("parent_id", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", 4)])   # 48 bytes
VOC_WORD_DTYPE = np.dtype([("node_id", "<i4"), ("word_id", "<i4")])
assert VOC_NODE_DTYPE.itemsize == 48 and VOC_WORD_DTYPE.itemsize == 8


class Vocabulary:
    """The content of the reference's binary vocabulary file (ThirdParty/VocabularyBinary.hpp): k, L, scoring, weighting, the
    nodes in file order (a node's children are in this order; the root, node 0, is not listed) and the (node, word) pairs.
    Nothing is validated here: LoopDetector.set_vocabulary / load_vocabulary refuse what the library refuses."""

    def __init__(self, k, L, node_id, parent_id, weight, descriptor, word_node, word_id, scoring=L1_NORM, weighting=TF_IDF):
        self.k, self.L, self.scoring, self.weighting = int(k), int(L), int(scoring), int(weighting)
        self.node_id = np.ascontiguousarray(node_id, np.int32).reshape(-1)
        self.parent_id = np.ascontiguousarray(parent_id, np.int32).reshape(-1)
        self.weight = np.ascontiguousarray(weight, np.float64).reshape(-1)
        self.descriptor = np.ascontiguousarray(descriptor, np.uint64).reshape(-1, 4)
        self.word_node = np.ascontiguousarray(word_node, np.int32).reshape(-1)
        self.word_id = np.ascontiguousarray(word_id, np.int32).reshape(-1)
        n = len(self.node_id)
        if not (len(self.parent_id) == len(self.weight) == len(self.descriptor) == n and len(self.word_node) == len(self.word_id)):
            raise ValueError("Vocabulary: arrays of different lengths")

    def to_file(self, path):
        nodes = np.zeros(len(self.node_id), VOC_NODE_DTYPE)
        nodes["node_id"], nodes["parent_id"], nodes["weight"], nodes["descriptor"] = self.node_id, self.parent_id, self.weight, self.descriptor
        words = np.zeros(len(self.word_id), VOC_WORD_DTYPE)
        words["node_id"], words["word_id"] = self.word_node, self.word_id
        with open(path, "wb") as f:
            f.write(np.array([self.k, self.L, self.scoring, self.weighting, len(nodes), len(words)], "<i4").tobytes())
            f.write(nodes.tobytes())
            f.write(words.tobytes())

    @classmethod
    def from_file(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < 24:
            raise ValueError("vocabulary file truncated inside its header")
        k, L, scoring, weighting, n, w = (int(x) for x in np.frombuffer(raw, "<i4", 6))
        if n < 0 or w < 0 or len(raw) < 24 + 48 * n + 8 * w:
            raise ValueError("vocabulary file truncated: %d bytes for %d nodes and %d words" % (len(raw), n, w))
        nodes = np.frombuffer(raw, VOC_NODE_DTYPE, n, 24)
        words = np.frombuffer(raw, VOC_WORD_DTYPE, w, 24 + 48 * n)
        return cls(k, L, nodes["node_id"], nodes["parent_id"], nodes["weight"], nodes["descriptor"], words["node_id"], words["word_id"],
                   scoring, weighting)


class LoopDetectorOptions(C.Structure):
    """vpl_ld_options"""
    _fields_ = [("max_keyframes", C.c_int), ("max_keypoints", C.c_int), ("max_words_total", C.c_int), ("max_results", C.c_int),
                ("recent", C.c_int), ("neighbour_score", C.c_double), ("loop_score", C.c_double)]


class LoopDetectorResult(C.Structure):
    """vpl_ld_result"""
    _fields_ = [("loop_index", C.c_int), ("n_results", C.c_int), ("ids", C.c_int * 4), ("scores", C.c_double * 4),
                ("n_words", C.c_int), ("entry", C.c_int)]


def _bind_ld(lib):
    if getattr(lib, "_vpl_ld_bound", False):
        return
    vp, ip, dp, u64p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
    rp = C.POINTER(LoopDetectorResult)
    lib.vpl_ld_default_options.argtypes = [C.POINTER(LoopDetectorOptions)]
    lib.vpl_ld_default_options.restype = None
    lib.vpl_ld_create.argtypes = [C.POINTER(vp), vp, C.c_int, C.POINTER(LoopDetectorOptions)]
    lib.vpl_ld_destroy.argtypes = [vp]
    lib.vpl_ld_destroy.restype = None
    lib.vpl_ld_set_vocabulary.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, dp, u64p, C.c_int, ip, ip]
    lib.vpl_ld_load_vocabulary.argtypes = [vp, C.c_char_p]
    lib.vpl_ld_detect.argtypes = [vp, u64p, ip, ip, rp]
    lib.vpl_ld_detect_fe.argtypes = [vp, ip, rp]
    lib.vpl_ld_add.argtypes = [vp, u64p, ip, rp]
    lib.vpl_ld_reset.argtypes = [vp, C.c_int]
    lib.vpl_ld_size.argtypes = [vp, C.c_int]
    lib.vpl_ld_get_bow.argtypes = [vp, C.c_int, C.c_int, ip, ip, dp]
    lib._vpl_ld_bound = True


def default_loop_detector_options(**kw):
    """vpl_ld_default_options (detectLoop's constants: 4 results, the 50 most recent keyframes left out, scores 0.05 / 0.015) with
    any field given by name filled in"""
    lib = load_hip_library()
    _bind_ld(lib)
    o = LoopDetectorOptions()
    lib.vpl_ld_default_options(C.byref(o))
    for k, val in kw.items():
        setattr(o, k, val)
    return o


class LoopDetector:
    """vpl_ld_*: the vocabulary, n_db keyframe databases and detectLoop on the device.  Borrows a FrontendContext; detect_fe takes
    the descriptor rows its last lc_keyframe left on the device (lc_reserve with the session's max_keypoints)."""

    def __init__(self, fe, n_db, options=None, **kw):
        self.fe, self.lib, self.n_db = fe, fe.lib, n_db
        _bind_ld(self.lib)
        self.opt = options or default_loop_detector_options(**kw)
        self.h = C.c_void_p()
        fe._check(self.lib.vpl_ld_create(C.byref(self.h), fe.h, n_db, C.byref(self.opt)), "vpl_ld_create")
        fe._ld = self
        self._res = (LoopDetectorResult * n_db)()

    def close(self):
        if self.h:
            self.lib.vpl_ld_destroy(self.h)
            self.h = C.c_void_p()
            if getattr(self.fe, "_ld", None) is self:
                self.fe._ld = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_vocabulary(self, voc):
        ip, dp, u64 = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
        self.fe._check(self.lib.vpl_ld_set_vocabulary(
            self.h, voc.k, voc.L, voc.scoring, voc.weighting, len(voc.node_id), voc.node_id.ctypes.data_as(ip),
            voc.parent_id.ctypes.data_as(ip), voc.weight.ctypes.data_as(dp), voc.descriptor.ctypes.data_as(u64), len(voc.word_id),
            voc.word_node.ctypes.data_as(ip), voc.word_id.ctypes.data_as(ip)), "vpl_ld_set_vocabulary")

    def load_vocabulary(self, path):
        self.fe._check(self.lib.vpl_ld_load_vocabulary(self.h, os.fsencode(path)), "vpl_ld_load_vocabulary")

    def _rows(self, briefs):
        """per database a [m][4] uint64 array, or None to leave the database untouched -> (rows, counts)"""
        assert len(briefs) == self.n_db
        MK = self.opt.max_keypoints
        rows, cnt = np.zeros((self.n_db, MK, 4), np.uint64), np.zeros(self.n_db, np.int32)
        for d, b in enumerate(briefs):
            if b is None:
                cnt[d] = -1
                continue
            b = np.asarray(b, np.uint64).reshape(-1, 4)
            cnt[d] = len(b)
            if len(b) <= MK:            # otherwise the library reports VPL_E_CAPACITY
                rows[d, :len(b)] = b
        return rows, cnt

    def _results(self):
        out = []
        for d in range(self.n_db):
            r = self._res[d]
            n = r.n_results
            out.append(dict(loop_index=r.loop_index, ids=np.array(r.ids[:n], np.int32), scores=np.array(r.scores[:n], np.float64),
                            n_words=r.n_words, entry=r.entry))
        return out

    def detect(self, briefs, frame_index):
        """detectLoop for every database: briefs as for _rows, frame_index [n_db] -> per database a dict: loop_index, ids and
        scores [n_results], n_words of the new bag, entry (the id the keyframe got; -1 for a database left untouched)"""
        rows, cnt = self._rows(briefs)
        fi = np.ascontiguousarray(frame_index, np.int32)
        assert fi.shape == (self.n_db,)
        ip = C.POINTER(C.c_int)
        self.fe._check(self.lib.vpl_ld_detect(self.h, rows.ctypes.data_as(C.POINTER(C.c_ulonglong)), cnt.ctypes.data_as(ip),
                                              fi.ctypes.data_as(ip), self._res), "vpl_ld_detect")
        return self._results()

    def detect_fe(self, frame_index):
        """detect on the rows the context's last lc_keyframe left on the device: image slot i goes to database i"""
        fi = np.ascontiguousarray(frame_index, np.int32)
        assert fi.shape == (self.n_db,)
        self.fe._check(self.lib.vpl_ld_detect_fe(self.h, fi.ctypes.data_as(C.POINTER(C.c_int)), self._res), "vpl_ld_detect_fe")
        return self._results()

    def add(self, briefs):
        """addKeyFrameIntoVoc: the bags join their databases without a query"""
        rows, cnt = self._rows(briefs)
        self.fe._check(self.lib.vpl_ld_add(self.h, rows.ctypes.data_as(C.POINTER(C.c_ulonglong)), cnt.ctypes.data_as(C.POINTER(C.c_int)),
                                           self._res), "vpl_ld_add")
        return self._results()

    def reset(self, db):
        self.fe._check(self.lib.vpl_ld_reset(self.h, db), "vpl_ld_reset")

    def size(self, db):
        n = self.lib.vpl_ld_size(self.h, db)
        if n < 0:
            raise ValueError("LoopDetector.size: no database %d" % db)
        return n

    def bow(self, db, entry):
        """test access: (words int32 ascending, values float64) of a stored bag"""
        MK = self.opt.max_keypoints
        n = C.c_int(0)
        w, val = np.zeros(MK, np.int32), np.zeros(MK, np.float64)
        self.fe._check(self.lib.vpl_ld_get_bow(self.h, db, entry, C.byref(n), w.ctypes.data_as(C.POINTER(C.c_int)),
                                               val.ctypes.data_as(C.POINTER(C.c_double))), "vpl_ld_get_bow")
        return w[:n.value].copy(), val[:n.value].copy()
