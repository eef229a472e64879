"""What the Gaussian tools share on the host: the shared command-line options, which views a run works on, the camera and
render size of a view (the one rule every tool depends on), the device guard, the point cloud on the device and the draw of
a step's views.  A new Gaussian tool starts here; render_gaussian_features.py is the smallest example.

Importing this module pulls in the standard library and numpy only (tests/test_gaussian_views_cpu.py holds that), so
query_voxel_features.build_parser can use it; torch and the project's heavier modules are imported by the functions that
need them.
"""
import numpy as np

import gaussian_ply

MAX_WIDTH = 1600


def render_size(W0, H0, downsample_factor=None):
    """(W, H): 3DGS's -r -1 rule (widths above 1600 down to 1600, int() of the scaled size), or int(W0 * f) x int(H0 * f)."""
    if downsample_factor is not None:
        return int(W0 * downsample_factor), int(H0 * downsample_factor)
    scale = W0 / MAX_WIDTH if W0 > MAX_WIDTH else 1.0
    return int(W0 / scale), int(H0 / scale)


def camera(entry, cams, W0, H0, W, H, principal_point="center"):
    """(viewmat f64 [4,4] = [R | tvec], K f64 [3,3]) at the render size: focal lengths scaled by W/W0 and H/H0 (the
    reference's focal = W / (2 tan(FoVx / 2)) with FoVx from the original focal and width); principal point at (W/2, H/2)
    or, with principal_point='camera', the camera's own scaled to the image."""
    params = cams[str(entry["camera_id"])]["params"]
    if len(params) == 4:
        fx, fy, cx, cy = (float(v) for v in params)
    else:
        fx, cx, cy = (float(v) for v in params)
        fy = fx
    sx, sy = W / W0, H / H0
    if principal_point == "camera":
        ppx, ppy = cx * sx, cy * sy
    else:
        ppx, ppy = W / 2.0, H / 2.0
    K = np.array([[fx * sx, 0.0, ppx], [0.0, fy * sy, ppy], [0.0, 0.0, 1.0]])
    vm = np.eye(4)
    vm[:3, :3] = np.asarray(entry["R"], np.float64)
    vm[:3, 3] = np.asarray(entry["tvec"], np.float64)
    return vm, K


def add_view_arguments(ap, images_help=None, views_help="image names (default: all, sorted)"):
    """The seven options that name the Gaussians, the cameras and the views.  ``images_help``: the tool reads the images
    themselves, so --images_dir is required and described by this text (their size then comes from the camera)."""
    ap.add_argument("--gaussians_ply", required=True, help="3DGS point_cloud.ply (binary little-endian)")
    ap.add_argument("--cam_params", required=True, help="camera_params.json")
    if images_help:
        ap.add_argument("--images_dir", required=True, help=images_help)
    else:
        ap.add_argument("--images_dir", default="", help="the images, for their size (else the camera's width / height)")
    ap.add_argument("--views", nargs="*", default=None, help=views_help)
    ap.add_argument("--max_images", type=int, default=None, help="only the first N of those views")
    ap.add_argument("--downsample_factor", type=float, default=None, help="override the 1600-pixel width rule")
    ap.add_argument("--principal_point", choices=("center", "camera"), default="center")


def view_names(views, default, max_images):
    """The views a run works on: the names given, in their order, or else the default set (the camera entries, or the
    masks) sorted; then the first ``max_images`` of them.  May be empty: what that means is the caller's to say."""
    names = list(views) if views else sorted(default)
    return names if max_images is None else names[:max_images]


def view_camera(entry, cams, name, images_dir, downsample_factor, principal_point):
    """(viewmat, K, W, H) of the camera entry of view ``name``; KeyError when ``entry`` is None.  The original size is the
    image's in ``images_dir`` when it is there, else the camera's own."""
    import aggregate_voxel_features_onthefly as agg
    if entry is None:
        raise KeyError(f"no camera entry for {name}")
    H0, W0 = agg._image_size(entry, cams, images_dir, name)
    W, H = render_size(W0, H0, downsample_factor)
    vm, K = camera(entry, cams, W0, H0, W, H, principal_point)
    return vm, K, W, H


def open_views(args, images_dir=None):
    """(names, view): the views of a parsed command line and ``view(name)`` -> (viewmat, K, W, H).  ``images_dir``
    replaces args.images_dir as the place the sizes are looked up in."""
    import prepare_tensor_data as ptd
    by_name, cams = ptd.load_camera_params(args.cam_params)
    if images_dir is None:
        images_dir = args.images_dir

    def view(name):
        return view_camera(by_name.get(name), cams, name, images_dir, args.downsample_factor, args.principal_point)

    return view_names(args.views, by_name, args.max_images), view


def iter_views(args):
    """(name, viewmat, K, W, H) of every requested view, each worked out when the loop reaches it."""
    names, view = open_views(args)
    if not names:
        raise ValueError("no views to render")
    for name in names:
        yield (name,) + view(name)


def open_mask_views(args, dev):
    """(names, load_view) of the tools that train on instance masks: the default views are the .png masks of
    args.masks_dir, every name is checked for its mask and its camera before anything is loaded, and ``load_view(name)`` ->
    (viewmat, K, W, H, ids int32 [H,W] on ``dev``, brought to the render size by nearest neighbour) keeps what it loaded:
    the masks are small, so they stay on the device."""
    import torch

    import evaluate_label_maps as elm
    import prepare_tensor_data as ptd
    by_name, cams = ptd.load_camera_params(args.cam_params)
    masks = {k: v for k, v in elm.index_dir(args.masks_dir).items() if v.lower().endswith(".png")}
    names = view_names(args.views, masks, args.max_images)
    if not names:
        raise ValueError(f"{args.masks_dir}: no .png masks to train on")
    for name in names:
        if name not in masks:
            raise KeyError(f"{args.masks_dir}: no mask for view '{name}'")
        if name not in by_name:
            raise KeyError(f"{args.cam_params}: no camera entry for {name}")
    cache = {}

    def load_view(name):
        if name not in cache:
            vm, K, W, H = view_camera(by_name[name], cams, name, args.images_dir, args.downsample_factor, args.principal_point)
            ids = elm.load_label_map(masks[name])
            if ids.shape != (H, W):
                ids = elm.resize_nearest(ids, W, H)
            cache[name] = (vm, K, W, H, torch.from_numpy(ids).to(dev))
        return cache[name]

    return names, load_view


def require_gpu(tool):
    """The current CUDA device; ``tool`` names the program in the refusal."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"{tool} runs on the GPU: there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def load_gaussians(path, dev):
    """The point cloud's activated arrays (gaussian_ply.read_gaussian_ply) as tensors on ``dev``."""
    import torch
    return {k: torch.from_numpy(v).to(dev) for k, v in gaussian_ply.read_gaussian_ply(path).items()}


def draw_indices(n, k, gen):
    """A step's pick: the first k of one torch.randperm(n) of the generator, as a list (one draw of ``gen`` per call)."""
    import torch
    return torch.randperm(n, generator=gen)[:k].tolist()
