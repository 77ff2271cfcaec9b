#!/usr/bin/python3
"""Series inference from the command line: a raw HU volume in, the synthesized CTA volume out.

    python predict.py --config Yaml/HdGan.yaml --weights netG_A2B.pth --input series.npy --output out.npy
                      [--level-dir DIR] [--hu] [--wc 50 --ww 400] [--batch 16] [--dtype bf16x3]
                      [--mip-dir DIR [--mip-mode max|min|mean] [--slab K] [--aspect R]]
                      [--rot-dir DIR [--rot-angles 36] [--rot-span 360] [--rot-sampling nearest|bilinear] [--rot-oversample S]
                       [--mip-mode max|min|mean] [--aspect R]]
                      [--sts-dir DIR --sts-thick T[,Tc,Ts] [--sts-step S[,Sc,Ss]] [--sts-axes axial,coronal,sagittal]
                       [--mip-mode max|min|mean] [--aspect R]]
                      [--sub-output sub.npy [--sub-level-dir DIR] [--sub-floor 0] [--sub-no-median] [--sub-ct-min HU]
                       [--sub-ct-max HU] [--sub-wc 150 --sub-ww 300] [--mip-source cta|sub]]
                      [--depth [--depth-cue C]]
                      [--vr-dir DIR [--vr-angles 36] [--vr-span 360] [--vr-preset grey|vessels|bone] [--vr-wc 300 --vr-ww 1500]
                       [--vr-sampling nearest|bilinear] [--vr-oversample S] [--vr-background R,G,B] [--aspect R]]
                      [--vr3d-dir DIR [--vr3d-axis x|y|z|X,Y,Z] [--vr3d-sampling nearest|trilinear]
                       [--vr3d-shade [--vr3d-ambient 0.3] [--vr3d-gmin 40]]]
                      [--mpr-dir DIR --mpr-normal X,Y,Z [--mpr-count P] [--mpr-pitch D] [--mpr-thick T]]
                      [--tumble-dir DIR [--tumble-angles 36] [--tumble-axis x|y|z]]
                      [--cpr-dir DIR --cpr-centreline pts.npy [--cpr-angles A] [--cpr-width U] [--cpr-thick T]]
                      [--cl-start Z,Y,X --cl-end Z,Y,X [--cl-end ...] --cl-threshold LO[,HI] [--cl-radius R] [--cl-output pts.npy]]
                      [--lumen-output lumen.npz [--lumen-rays K] [--lumen-reach PX] [--lumen-oversample S]
                       [--lumen-edge band|half --lumen-base HU] [--lumen-recentre I] [--pixel-mm MM]]
                      [--reformat-sampling nearest|trilinear]
                      [--cc-output vessels.npy --cc-threshold LO[,HI] [--cc-level-dir DIR] [--cc-connectivity 6|18|26]
                       [--cc-min-voxels M] [--cc-largest K] [--cc-seed Z,Y,X ...] [--cc-despeckle] [--cc-source cta|sub]
                       [--cc-labels labels.npy] [--mip-source vessels]]

--input: int16 [N, H, W] .npy in SimpleITK's convention (what the reference's loaders read from the DICOMs); --weights: the
reference-format `state_dict` of Model.HdGan.Generator (what train() saves as netG_A2B*.pth).  --output receives the int16
volume the reference's test() writes into the DICOMs (trainer/HdTrainer.py:539-543; --hu: minus 1024, SimpleITK's convention
again); --level-dir one 8-bit PNG per slice of the window (--wc, --ww).  The generator runs at config['size']; a series of
another size is resized on the way in and comes back at its own.  --mip-dir: the projections of the synthesized volume along
the three body axes (--mip-mode: maximum, minimum or mean intensity), accumulated on the device while the volume is made:
axial_%03d.png (one per slab of --slab slices; without --slab the whole volume, axial_000.png), coronal.png and sagittal.png in
the window, and projections.npz with the int16 values (axial [S, H, W], coronal [N, W], sagittal [N, H]).  --aspect R = slice
spacing / pixel spacing draws the coronal and sagittal PNGs with round(N R) rows (nearest; the .npz keeps N rows).
--rot-dir: the rotating projection of the synthesized volume, --rot-angles views over --rot-span degrees about the cranio-caudal
axis (0 = coronal, 90 = sagittal; --mip-mode, --wc / --ww, --hu and --aspect as above), made on the device while the volume is
made: rot_%03d.png, one 8-bit frame [round(N R), D] per angle with D = ceil(hypot(H, W)), and rotation.npz with values (int16
[A, N, D]), level (uint8) and angles (degrees).  --rot-sampling bilinear interpolates the four pixels around every sample of a
ray instead of taking the nearest one, and --rot-oversample S takes S steps per voxel (with either sampling): a one-pixel vessel
that nearest sampling at unit steps steps over at some angles is seen at every angle by bilinear, at nearly every one by S = 2.
--sts-dir: the sliding thin-slab projections of the synthesized volume, the mode a CTA is read in: slabs of --sts-thick voxels
moved on by --sts-step voxels (default: the thickness, slabs that do not overlap; 1 <= step <= thick) along the --sts-axes.  One
number serves every axis, three (axial, coronal, sagittal) give each axis its own: slice spacing and pixel spacing differ.
axial_%03d.png [H, W], coronal_%03d.png [round(N R), W] and sagittal_%03d.png [round(N R), H], one per slab, in the window
(--mip-mode, --wc / --ww, --hu and --aspect as above), and slabs.npz with the int16 values per axis.
--sub-output: the subtraction volume, synthesized CTA minus the input CT (int16 [N, H, W] .npy of HU differences), made on the
device while the volume is made: the pair is registered by construction, so bone cancels.  A 3 x 3 in-plane median unless
--sub-no-median; differences below --sub-floor, and pixels whose input HU lies outside --sub-ct-min .. --sub-ct-max (default:
open), become 0.  --sub-level-dir: one 8-bit PNG per slice in the window --sub-wc / --sub-ww of a HU difference.  --mip-source
sub makes --mip-dir, --rot-dir, --sts-dir and --vr-dir show the subtraction volume (levels in the --sub window) instead of the synthesized one: the
bone-free MIP.
--depth (with --mip-dir and / or --rot-dir, --mip-mode max or min): the depth of the maximum.  rotation.npz gains depth (int16
[A, N, D]: the step along the ray, counted from the viewer's end, at which the value was found; -1 where the ray misses the
slice) and projections.npz gains axial_depth, coronal_depth and sagittal_depth (the slice, row or column of the value).
--depth-cue C (0 .. 256, default 0) also adds the depth-cued levels (cued; axial_cued, coronal_cued, sagittal_cued): the level
attenuated by up to C / 256 toward the far end of the ray, which tells front from back in the rotating view; with C > 0 the PNGs
are written from them.  Without --depth every output is what it was.
--vr-dir: the volume-rendered rotating view of the same source (--mip-source), --vr-angles views over --vr-span degrees, made on
the device while the volume is made: every ray is composited front to back, so what lies in front hides what lies behind.  A
sample's class is its 8-bit level in the transfer window --vr-wc / --vr-ww (independent of --wc / --ww); --vr-preset names the
transfer function that gives every class its colour and opacity (cta_gan_amd/infer.py: TRANSFER_PRESETS).  --vr-sampling and
--vr-oversample as --rot-sampling and --rot-oversample (the opacities are corrected per step); --vr-background R,G,B (0 .. 255)
shows through where a ray stays transparent.  vr_%03d.png, one RGB frame [round(N R), D] per angle, and render.npz with rgb
(uint8 [A, N, D, 3]), opacity (uint8), depth (int16: the step at which a ray becomes half opaque, -1 if never), angles and lut
(the uint16 [256, 4] transfer table that was used).
--vr3d-dir: the volume-rendered view along rays in any direction, made after the last chunk from the volume kept on the device
(cta_gan_amd/infer.py: VolumeRenderer): --vr-angles views over --vr-span degrees about --vr3d-axis x (default: the tumble), y, z
or any X,Y,Z through the centre, with --vr-preset, --vr-wc / --vr-ww, --vr-oversample, --vr-background and --mip-source as for
--vr-dir and --vr3d-sampling trilinear (default) or nearest.  --aspect R is inside the geometry: the frames are isotropic and no
row is repeated.  --vr3d-shade shades every sample by the local gradient under a light along the rays: --vr3d-ambient (0 .. 1)
is the share of its colour a wall edge-on to the light keeps, --vr3d-gmin the gradient (stored units over two voxels) below
which a sample keeps its colour.  vr3d_%03d.png, one RGB frame per angle, and render3d.npz with rgb (uint8 [A, R, U, 3]), opacity
(uint8), depth (int16), angles, lut, lines (the int64 [A, R, 9] line table) and light (int64 [A, R, 3]; empty without
--vr3d-shade).
--mpr-dir, --tumble-dir, --cpr-dir: reformats whose rows cross slices, made after the last chunk from the volume kept on the
device (cta_gan_amd/infer.py: VolumeReformatter), of the same source (--mip-source) in the same window, with --mip-mode along
their rays and --reformat-sampling trilinear (default) or nearest.  --aspect R is inside their geometry: the images are isotropic
and no row is repeated.  --mpr-dir: --mpr-count parallel oblique planes with the normal --mpr-normal X,Y,Z (x = column, y = row,
z = slice), --mpr-pitch pixels apart and centred on the volume, each a slab --mpr-thick voxels deep (1: a plain plane):
mpr_%03d.png.  --tumble-dir: the rotating projection about another axis than --rot-dir's, --tumble-angles views around the full
circle about --tumble-axis x (default: the tumble), y or z through the centre: tumble_%03d.png.  --cpr-dir: the straightened
curved reformat along --cpr-centreline (a .npy of M >= 2 points (z, y, x) in voxels), --cpr-width samples across the vessel,
--cpr-angles views around it, slabs --cpr-thick voxels deep: cpr_%03d.png.  Each directory also receives reformat.npz with values
(int16), level (uint8) and, for the rotating kinds, angles (degrees).
--cc-output: the volume with only the wanted connected components left (int16 [N, H, W] .npy), made on the device after the
last chunk (cta_gan_amd/infer.py: VolumeComponents).  A voxel is foreground when --cc-threshold LO <= value <= HI (default HI:
32767; stored values of --cc-source cta, the default, or HU differences of --cc-source sub, which needs --sub-output);
--cc-connectivity 6, 18 or 26 (default) joins foreground voxels by faces, faces and edges, or all 26 neighbours.  Kept are the
components of at least --cc-min-voxels voxels, of those only the ones a --cc-seed Z,Y,X (repeatable: the voxel a click on a MIP
maps to) lies in, of those the --cc-largest K biggest (0: all).  Everything else becomes air; with --cc-despeckle the background
keeps its values and only the dropped components are erased.  --cc-level-dir: one 8-bit PNG per slice in the source's window;
--cc-labels: the int32 label volume (-1 on background, otherwise the smallest linear index of the voxel's component).  Next to
--cc-output, components.npz holds top (int32 [8, 2]: root and size of the biggest kept components, (-1, 0) beyond them), stats
(int32 [8]) and roots_zyx (the voxel of every root in top, -1 where there is none), and one line reports the components found,
kept and the voxels kept.  --mip-source vessels makes --mip-dir, --rot-dir, --sts-dir, --vr-dir and the reformats show that
cleaned volume, in the window of its source.
--cl-start Z,Y,X with one or more --cl-end Z,Y,X: the vessel centreline from the start voxel to every end voxel (the voxels clicks
on a MIP or a rendered view map to; they must lie on foreground), traced on the device after the last chunk through the same
source as the other displays (cta_gan_amd/infer.py: VolumeCentreline): the cheapest path through the voxels with --cl-threshold
LO <= value <= HI (default HI: 32767) when a step costs more the closer it runs to the vessel wall, the distance to the wall
capped at --cl-radius R pixels (default 8); --aspect R scales z.  --cl-output pts.npy receives the smoothed points (float64
[M, 3], (z, y, x), start to end) of the first end -- what --cpr-centreline reads -- and centreline.npz next to it (next to
--output without it) paths, counts, stats and points_0, points_1, ... of every end; one line reports the lengths.  --cpr-dir
without --cpr-centreline then makes the curved reformat along the traced line of the first end in the same run.
--lumen-output lumen.npz (with --cl-start): the lumen measured along the traced line of every end in the same run
(cta_gan_amd/infer.py: VolumeCentreline(lumen=...), lumen_profile, lumen_stenosis): --lumen-rays K = 8, 16, 32 or 64 rays across
the vessel at every pixel of arc length, walked out to --lumen-reach pixels in steps of 1 / --lumen-oversample until the value
leaves the band of --cl-threshold; --lumen-edge half puts the wall half-way between the section's own centre value and the
background --lumen-base (a stored value, not above LO) instead; --lumen-recentre I = 0 .. 4 moves every section's centre to the
middle of its own boundary first (without it the least diameter measures the click, not the vessel).  The file holds radii, cross,
sections, centres and, with --pixel-mm MM (the in-plane pixel spacing, default 1), area, equivalent, dmin, dmax, mean, arc and
valid of every end (suffix _0, _1, ...); one line per end reports the stenosis grade.  A branch leaves rays open: such sections
are not valid and take no part in the grade.
DICOM reading and writing are not part of this build.
"""
import argparse
import os

DTYPES = ["fp32", "bf16", "bf16x3", "bf16x3f"]
DEFAULT_DTYPE = "bf16x3"      # train.py's default
VR_PRESETS = ["grey", "vessels", "bone"]      # the names of cta_gan_amd.infer.TRANSFER_PRESETS (not imported here: --help needs no torch)


def build_parser():
    parser = argparse.ArgumentParser(description="HU series (.npy) -> synthesized CTA series (.npy)")
    parser.add_argument("--config", type=str, default="Yaml/HdGan.yaml", help="Path to the config file.")
    parser.add_argument("--weights", type=str, required=True, help="state_dict of Model.HdGan.Generator (.pth)")
    parser.add_argument("--input", type=str, required=True, help="int16 [N, H, W] .npy, raw HU")
    parser.add_argument("--output", type=str, required=True, help="int16 [N, H, W] .npy to write")
    parser.add_argument("--level-dir", type=str, default=None, help="also write one 8-bit PNG of the window per slice here")
    parser.add_argument("--hu", action="store_true", help="write HU (stored value - 1024) instead of stored values")
    parser.add_argument("--wc", type=float, default=50.0, help="window centre of the 8-bit level")
    parser.add_argument("--ww", type=float, default=400.0, help="window width of the 8-bit level")
    parser.add_argument("--batch", type=int, default=16, help="slices per generator forward")
    parser.add_argument("--mip-dir", type=str, default=None, help="also write the projections of the synthesized volume here")
    parser.add_argument("--mip-mode", choices=["max", "min", "mean"], default="max", help="projection (with --mip-dir)")
    parser.add_argument("--slab", type=int, default=None, help="slices per axial slab (default: the whole volume)")
    parser.add_argument("--aspect", type=float, default=1.0, help="slice spacing / pixel spacing of the coronal / sagittal PNGs")
    parser.add_argument("--rot-dir", type=str, default=None, help="also write the rotating projection of the synthesized volume here")
    parser.add_argument("--rot-angles", type=int, default=36, help="view angles of the rotating projection (with --rot-dir)")
    parser.add_argument("--rot-span", type=float, default=360.0, help="degrees the view angles are spread over (with --rot-dir)")
    parser.add_argument("--rot-sampling", choices=["nearest", "bilinear"], default="nearest", help="how a ray samples the slice (with --rot-dir)")
    parser.add_argument("--rot-oversample", type=int, default=1, help="steps per voxel along a ray (with --rot-dir)")
    parser.add_argument("--depth", action="store_true", help="also record the depth of the maximum (with --mip-dir / --rot-dir)")
    parser.add_argument("--depth-cue", type=int, default=0, help="0 .. 256: attenuate the levels by depth (with --depth)")
    parser.add_argument("--vr-dir", type=str, default=None, help="also write the volume-rendered rotating view here")
    parser.add_argument("--vr-angles", type=int, default=36, help="view angles of the rendered view (with --vr-dir)")
    parser.add_argument("--vr-span", type=float, default=360.0, help="degrees the view angles are spread over (with --vr-dir)")
    parser.add_argument("--vr-preset", choices=VR_PRESETS, default="vessels", help="transfer function (with --vr-dir)")
    parser.add_argument("--vr-wc", type=float, default=300.0, help="centre of the transfer function's window (with --vr-dir)")
    parser.add_argument("--vr-ww", type=float, default=1500.0, help="width of the transfer function's window (with --vr-dir)")
    parser.add_argument("--vr-sampling", choices=["nearest", "bilinear"], default="nearest", help="how a ray samples the slice (with --vr-dir)")
    parser.add_argument("--vr-oversample", type=int, default=1, help="steps per voxel along a ray (with --vr-dir)")
    parser.add_argument("--vr-background", type=str, default="0,0,0", help="R,G,B in 0 .. 255 behind the rendered view (with --vr-dir)")
    parser.add_argument("--vr3d-dir", type=str, default=None, help="also write the volume-rendered view about --vr3d-axis here")
    parser.add_argument("--vr3d-axis", type=str, default="x", help="the axis of the orbit: x, y, z or X,Y,Z (with --vr3d-dir)")
    parser.add_argument("--vr3d-sampling", choices=["nearest", "trilinear"], default="trilinear",
                        help="how a ray samples the volume (with --vr3d-dir)")
    parser.add_argument("--vr3d-shade", action="store_true", help="shade every sample by the local gradient (with --vr3d-dir)")
    parser.add_argument("--vr3d-ambient", type=float, default=0.3, help="the share of its colour an unlit wall keeps (with --vr3d-shade)")
    parser.add_argument("--vr3d-gmin", type=float, default=40.0, help="the gradient below which a sample is not shaded (with --vr3d-shade)")
    parser.add_argument("--mpr-dir", type=str, default=None, help="also write oblique planes (MPR) here")
    parser.add_argument("--mpr-normal", type=str, default=None, help="X,Y,Z: the normal of the oblique planes (with --mpr-dir)")
    parser.add_argument("--mpr-count", type=int, default=1, help="parallel oblique planes (with --mpr-dir)")
    parser.add_argument("--mpr-pitch", type=float, default=1.0, help="pixels between two oblique planes (with --mpr-dir)")
    parser.add_argument("--mpr-thick", type=int, default=1, help="voxels an oblique plane is deep: a slab (with --mpr-dir)")
    parser.add_argument("--tumble-dir", type=str, default=None, help="also write the projection rotating about --tumble-axis here")
    parser.add_argument("--tumble-angles", type=int, default=36, help="view angles around the full circle (with --tumble-dir)")
    parser.add_argument("--tumble-axis", choices=["x", "y", "z"], default="x", help="the axis of the orbit (with --tumble-dir)")
    parser.add_argument("--cpr-dir", type=str, default=None, help="also write the straightened curved reformat here")
    parser.add_argument("--cpr-centreline", type=str, default=None, help=".npy of M >= 2 points (z, y, x) in voxels (with --cpr-dir)")
    parser.add_argument("--cpr-angles", type=int, default=1, help="views around the centreline (with --cpr-dir)")
    parser.add_argument("--cpr-width", type=int, default=65, help="samples across the vessel (with --cpr-dir)")
    parser.add_argument("--cpr-thick", type=int, default=1, help="voxels the curved reformat is deep: a slab (with --cpr-dir)")
    parser.add_argument("--reformat-sampling", choices=["nearest", "trilinear"], default="trilinear",
                        help="how --mpr-dir, --tumble-dir and --cpr-dir sample the volume")
    parser.add_argument("--sts-dir", type=str, default=None, help="also write the sliding thin-slab projections here")
    parser.add_argument("--sts-thick", type=str, default=None, help="voxels per slab: T, or T,Tc,Ts for axial,coronal,sagittal")
    parser.add_argument("--sts-step", type=str, default=None, help="voxels a slab moves on: S or S,Sc,Ss (default: the thickness)")
    parser.add_argument("--sts-axes", type=str, default="axial,coronal,sagittal", help="axes of --sts-dir, comma-separated")
    parser.add_argument("--sub-output", type=str, default=None, help="also write the subtraction volume (synthesized - input) here")
    parser.add_argument("--sub-level-dir", type=str, default=None, help="one 8-bit PNG per subtraction slice (with --sub-output)")
    parser.add_argument("--sub-floor", type=int, default=0, help="differences below this many HU become 0")
    parser.add_argument("--sub-no-median", action="store_true", help="skip the 3 x 3 in-plane median of the difference")
    parser.add_argument("--sub-ct-min", type=int, default=None, help="pixels whose input HU is below this become 0")
    parser.add_argument("--sub-ct-max", type=int, default=None, help="pixels whose input HU is above this become 0")
    parser.add_argument("--sub-wc", type=float, default=150.0, help="window centre of the subtraction's 8-bit level")
    parser.add_argument("--sub-ww", type=float, default=300.0, help="window width of the subtraction's 8-bit level")
    parser.add_argument("--mip-source", choices=["cta", "sub", "vessels"], default="cta", help="what --mip-dir / --rot-dir project")
    parser.add_argument("--cc-output", type=str, default=None, help="also write the volume with only the kept components here")
    parser.add_argument("--cc-level-dir", type=str, default=None, help="one 8-bit PNG per slice of it (with --cc-output)")
    parser.add_argument("--cc-threshold", type=str, default=None, help="LO or LO,HI: the foreground band (with --cc-output; a negative LO as --cc-threshold=-5,300)")
    parser.add_argument("--cc-connectivity", type=int, choices=[6, 18, 26], default=26, help="which neighbours join (with --cc-output)")
    parser.add_argument("--cc-min-voxels", type=int, default=1, help="drop components smaller than this (with --cc-output)")
    parser.add_argument("--cc-largest", type=int, default=0, help="keep only the K biggest components, 0: all (with --cc-output)")
    parser.add_argument("--cc-seed", type=str, action="append", default=None, help="Z,Y,X: keep the component of this voxel (repeatable)")
    parser.add_argument("--cc-despeckle", action="store_true", help="keep the background, erase only the dropped components")
    parser.add_argument("--cc-source", choices=["cta", "sub"], default=None, help="the volume the components are taken from")
    parser.add_argument("--cc-labels", type=str, default=None, help="also write the int32 label volume here (with --cc-output)")
    parser.add_argument("--cl-start", type=str, default=None, help="Z,Y,X: the voxel the vessel centreline starts at (with --cl-end)")
    parser.add_argument("--cl-end", type=str, action="append", default=None, help="Z,Y,X: a voxel a centreline is traced to (repeatable)")
    parser.add_argument("--cl-threshold", type=str, default=None, help="LO or LO,HI: the vessel's band (with --cl-start; as --cc-threshold)")
    parser.add_argument("--cl-radius", type=int, default=8, help="the clearance is capped at this many pixels, 1 .. 32 (with --cl-start)")
    parser.add_argument("--cl-output", type=str, default=None, help="write the smoothed centreline of the first end here (.npy, [M, 3])")
    parser.add_argument("--lumen-output", type=str, default=None, help="write the lumen profile along every traced centreline here (.npz; with --cl-start)")
    parser.add_argument("--lumen-rays", type=int, default=32, help="rays per cross-section: 8, 16, 32 or 64 (with --lumen-output)")
    parser.add_argument("--lumen-reach", type=float, default=16.0, help="how far a ray is walked, in pixels (with --lumen-output)")
    parser.add_argument("--lumen-oversample", type=int, default=2, help="steps per pixel along a ray (with --lumen-output)")
    parser.add_argument("--lumen-edge", type=str, default="band", choices=["band", "half"], help="the wall: where the value leaves the band, or half-way to --lumen-base")
    parser.add_argument("--lumen-base", type=int, default=None, help="the background's stored value (with --lumen-edge half)")
    parser.add_argument("--lumen-recentre", type=int, default=2, help="recentring moves per section, 0 .. 4 (with --lumen-output)")
    parser.add_argument("--pixel-mm", type=float, default=1.0, help="the in-plane pixel spacing in mm (with --lumen-output)")
    parser.add_argument("--dtype", choices=DTYPES, default=None, help="compute mode (default %s, as train.py)" % DEFAULT_DTYPE)
    return parser


STS_AXES = ("axial", "coronal", "sagittal")


def _sts_counts(parser, text, flag):
    """"T" or "T,Tc,Ts" -> {axis: int} over all three axes."""
    try:
        counts = [int(v) for v in text.split(",")]
    except ValueError:
        parser.error("%s: whole numbers expected, got %r" % (flag, text))
    if len(counts) not in (1, 3) or min(counts) < 1:
        parser.error("%s: one positive count, or three (axial,coronal,sagittal), expected, got %r" % (flag, text))
    return dict(zip(STS_AXES, counts * 3 if len(counts) == 1 else counts))


def sts_options(parser, opts):
    """The `SeriesTranslator(slabs=...)` dict of --sts-dir (None without it); bad values end in parser.error."""
    if opts.sts_dir is None:
        if opts.sts_thick is not None or opts.sts_step is not None:
            parser.error("--sts-thick and --sts-step need --sts-dir")
        return None
    if opts.sts_thick is None:
        parser.error("--sts-dir needs --sts-thick")
    axes = tuple(a for a in opts.sts_axes.split(",") if a)
    if not axes or any(a not in STS_AXES for a in axes) or len(set(axes)) != len(axes):
        parser.error("--sts-axes: a comma-separated choice of %s expected, got %r" % (", ".join(STS_AXES), opts.sts_axes))
    thick = _sts_counts(parser, opts.sts_thick, "--sts-thick")
    step = dict(thick) if opts.sts_step is None else _sts_counts(parser, opts.sts_step, "--sts-step")
    for a in axes:
        if step[a] > thick[a]:
            parser.error("--sts-step: %s step %d above its thickness %d" % (a, step[a], thick[a]))
    axes = tuple(a for a in STS_AXES if a in axes)
    return {"thick": {a: thick[a] for a in axes}, "step": {a: step[a] for a in axes}, "mode": opts.mip_mode, "axes": axes}


def _band(parser, flag, text):
    """"LO" or "LO,HI" -> (lo, hi) of a threshold band, hi = 32767 by default."""
    try:
        band = [int(v) for v in text.split(",")]
    except ValueError:
        parser.error("%s: whole numbers LO or LO,HI expected, got %r" % (flag, text))
    band = band + [32767] if len(band) == 1 else band
    if len(band) != 2 or not -32768 <= band[0] <= band[1] <= 32767:
        parser.error("%s: -32768 <= LO <= HI <= 32767 expected, got %r" % (flag, text))
    return tuple(band)


def _voxels(parser, flag, texts):
    """["Z,Y,X", ...] -> [(z, y, x), ...], whole numbers >= 0."""
    try:
        points = [tuple(int(v) for v in text.split(",")) for text in texts]
    except ValueError:
        parser.error("%s: whole numbers Z,Y,X expected, got %r" % (flag, texts))
    if any(len(p) != 3 or min(p) < 0 for p in points):
        parser.error("%s: three whole numbers Z,Y,X >= 0 expected, got %r" % (flag, texts))
    return points


def cc_options(parser, opts):
    """The `SeriesTranslator(components=...)` dict of --cc-output (None without it); bad values end in parser.error."""
    if opts.cc_output is None:
        if (opts.cc_threshold is not None or opts.cc_level_dir is not None or opts.cc_seed is not None or opts.cc_labels is not None
                or opts.cc_source is not None or opts.cc_despeckle or opts.mip_source == "vessels"):
            parser.error("the --cc options and --mip-source vessels need --cc-output")
        return None
    if opts.cc_threshold is None:
        parser.error("--cc-output needs --cc-threshold")
    if opts.cc_min_voxels < 1 or not 0 <= opts.cc_largest <= 64:
        parser.error("--cc-min-voxels: at least 1 and --cc-largest: 0 .. 64 expected")
    if opts.cc_source == "sub" and opts.sub_output is None:
        parser.error("--cc-source sub needs --sub-output")
    return {"threshold": _band(parser, "--cc-threshold", opts.cc_threshold), "connectivity": opts.cc_connectivity,
            "min_voxels": opts.cc_min_voxels, "largest": opts.cc_largest,
            "seeds": None if opts.cc_seed is None else _voxels(parser, "--cc-seed", opts.cc_seed), "background": opts.cc_despeckle,
            "level": opts.cc_level_dir is not None, "labels": opts.cc_labels is not None, "top": 8}


def cl_options(parser, opts):
    """The `SeriesTranslator(centreline=...)` dict of --cl-start / --cl-end (None without them); bad values end in parser.error."""
    if opts.cl_start is None and opts.cl_end is None:
        if opts.cl_threshold is not None or opts.cl_output is not None or opts.lumen_output is not None:
            parser.error("--cl-threshold, --cl-output and --lumen-output need --cl-start and --cl-end")
        return None
    if opts.cl_start is None or opts.cl_end is None or opts.cl_threshold is None:
        parser.error("--cl-start, --cl-end and --cl-threshold need each other")
    points = _voxels(parser, "--cl-start / --cl-end", [opts.cl_start] + opts.cl_end)
    if len(points) > 65:
        parser.error("--cl-end: at most 64 ends expected")
    if not 1 <= opts.cl_radius <= 32:
        parser.error("--cl-radius: 1 .. 32 expected")
    if not 0.25 <= opts.aspect < 16.0:
        parser.error("--aspect: 0.25 .. 16 expected with --cl-start")
    out = {"threshold": _band(parser, "--cl-threshold", opts.cl_threshold), "start": points[0], "ends": points[1:],
           "radius": opts.cl_radius, "aspect": opts.aspect}
    if opts.lumen_output is not None:
        steps = int(opts.lumen_reach * opts.lumen_oversample) + 1 if opts.lumen_oversample >= 1 and 0 < opts.lumen_reach < 1e6 else 0
        if opts.lumen_rays not in (8, 16, 32, 64) or not 2 <= steps <= 256 or not 0 <= opts.lumen_recentre <= 4 or not opts.pixel_mm > 0:
            parser.error("--lumen-rays: 8, 16, 32 or 64, --lumen-reach x --lumen-oversample: 1 .. 255 steps, --lumen-recentre: 0 .. 4 "
                         "and --pixel-mm above 0 expected")
        if (opts.lumen_edge == "half") != (opts.lumen_base is not None) or (opts.lumen_base is not None and opts.lumen_base > out["threshold"][0]):
            parser.error("--lumen-edge half and --lumen-base need each other, and the base must not lie above the LO of --cl-threshold")
        out["lumen"] = {"rays": opts.lumen_rays, "reach": opts.lumen_reach, "oversample": opts.lumen_oversample, "edge": opts.lumen_edge,
                        "base": opts.lumen_base, "recentre": opts.lumen_recentre}
    return out


def parse_args(argv=None):
    parser = build_parser()
    opts = parser.parse_args(argv)
    opts.sts = sts_options(parser, opts)
    opts.cc = cc_options(parser, opts)
    opts.cl = cl_options(parser, opts)
    if opts.sub_output is None and (opts.mip_source == "sub" or opts.sub_level_dir is not None):
        parser.error("--mip-source sub and --sub-level-dir need --sub-output")
    if opts.sub_ct_min is not None and opts.sub_ct_max is not None and opts.sub_ct_min > opts.sub_ct_max:
        parser.error("--sub-ct-min above --sub-ct-max")
    if not 0 <= opts.depth_cue <= 256:
        parser.error("--depth-cue: 0 .. 256 expected")
    if opts.depth_cue and not opts.depth:
        parser.error("--depth-cue needs --depth")
    if opts.depth and (opts.mip_mode == "mean" or (opts.mip_dir is None and opts.rot_dir is None)):
        parser.error("--depth needs --mip-dir or --rot-dir and --mip-mode max or min (a mean has no depth)")
    try:
        opts.vr_background = tuple(int(v) for v in opts.vr_background.split(","))
    except ValueError:
        parser.error("--vr-background: whole numbers R,G,B expected, got %r" % opts.vr_background)
    if len(opts.vr_background) != 3 or not all(0 <= v <= 255 for v in opts.vr_background):
        parser.error("--vr-background: three values R,G,B in 0 .. 255 expected")
    if opts.vr_angles < 1 or opts.vr_oversample < 1:
        parser.error("--vr-angles and --vr-oversample: at least 1 expected")
    if opts.vr3d_axis not in ("x", "y", "z"):
        try:
            opts.vr3d_axis = tuple(float(v) for v in opts.vr3d_axis.split(","))
        except ValueError:
            parser.error("--vr3d-axis: x, y, z or numbers X,Y,Z expected, got %r" % opts.vr3d_axis)
        if len(opts.vr3d_axis) != 3 or not any(opts.vr3d_axis):
            parser.error("--vr3d-axis: x, y, z or three numbers X,Y,Z, not all zero, expected")
    if not 0.0 <= opts.vr3d_ambient <= 1.0 or not 0.0 <= opts.vr3d_gmin <= 8192.0:
        parser.error("--vr3d-ambient: 0 .. 1 and --vr3d-gmin: 0 .. 8192 expected")
    if (opts.mpr_dir is None) != (opts.mpr_normal is None):
        parser.error("--mpr-dir and --mpr-normal need each other")
    if opts.mpr_normal is not None:
        try:
            opts.mpr_normal = tuple(float(v) for v in opts.mpr_normal.split(","))
        except ValueError:
            parser.error("--mpr-normal: numbers X,Y,Z expected, got %r" % opts.mpr_normal)
        if len(opts.mpr_normal) != 3 or not any(opts.mpr_normal):
            parser.error("--mpr-normal: three numbers X,Y,Z, not all zero, expected")
    if opts.mpr_count < 1 or opts.mpr_thick < 1 or not opts.mpr_pitch > 0:
        parser.error("--mpr-count and --mpr-thick: at least 1, --mpr-pitch: above 0 expected")
    if opts.tumble_angles < 1:
        parser.error("--tumble-angles: at least one view angle expected")
    opts.cpr_traced = opts.cpr_dir is not None and opts.cpr_centreline is None and opts.cl is not None
    if (opts.cpr_dir is None) != (opts.cpr_centreline is None) and not opts.cpr_traced:
        parser.error("--cpr-dir and --cpr-centreline need each other (or --cpr-dir with --cl-start / --cl-end: the traced centreline)")
    if opts.cpr_angles < 1 or opts.cpr_width < 1 or opts.cpr_thick < 1:
        parser.error("--cpr-angles, --cpr-width and --cpr-thick: at least 1 expected")
    if opts.cpr_traced:      # the curved reformat along the traced path of every end, made by the centreline view itself
        from cta_gan_amd.infer import view_angles
        opts.cl["cpr"] = {"angles": view_angles(opts.cpr_angles, 180.0), "cols": opts.cpr_width, "depth": opts.cpr_thick,
                          "sampling": opts.reformat_sampling, "mode": opts.mip_mode}
    return opts


def reformat_tables(opts):
    """The `SeriesTranslator(reformat=...)` tables of --mpr-dir / --tumble-dir / --cpr-dir by kind (None without any), and the
    view angles of the rotating kinds."""
    import numpy as np
    from cta_gan_amd.infer import curved_lines, oblique_lines, orbit_lines, view_angles
    tables, angles = {}, {}
    if opts.mpr_dir is not None:
        tables["mpr"] = lambda n, h, w: oblique_lines(n, h, w, opts.mpr_normal, count=opts.mpr_count, pitch=opts.mpr_pitch,
                                                      thick=opts.mpr_thick, aspect=opts.aspect)
    if opts.tumble_dir is not None:
        angles["tumble"] = view_angles(opts.tumble_angles)
        tables["tumble"] = lambda n, h, w: orbit_lines(n, h, w, angles["tumble"], axis=opts.tumble_axis, aspect=opts.aspect)
    if opts.cpr_dir is not None and not opts.cpr_traced:
        centreline = np.load(opts.cpr_centreline)
        angles["cpr"] = view_angles(opts.cpr_angles, 180.0)
        tables["cpr"] = lambda n, h, w: curved_lines(n, h, w, centreline, angles=angles["cpr"], cols=opts.cpr_width,
                                                     depth=opts.cpr_thick, aspect=opts.aspect)
    return (tables or None), angles


def write_pngs(where, pattern, planes, rows=None):
    """One PNG per plane (uint8 [H, W]: mode "L"; [H, W, 3]: "RGB") into the directory `where`, made if need be, named by
    `pattern` (of the plane's number, or the name of one plane); rows: the source row of every row of the picture."""
    import numpy as np
    from PIL import Image
    os.makedirs(where, exist_ok=True)
    for i, plane in enumerate(planes):
        name = pattern % i if "%" in pattern else pattern
        Image.fromarray(np.ascontiguousarray(plane if rows is None else plane[rows])).save(os.path.join(where, name))


def main(argv=None):
    opts = parse_args(argv)
    if opts.slab is not None and opts.slab < 1:
        raise SystemExit("--slab: at least one slice per slab expected")
    if opts.aspect <= 0:
        raise SystemExit("--aspect: a positive ratio expected")
    if opts.rot_dir is not None and opts.rot_angles < 1:
        raise SystemExit("--rot-angles: at least one view angle expected")
    if opts.rot_oversample < 1:
        raise SystemExit("--rot-oversample: at least one step per voxel expected")
    import numpy as np
    import torch
    import yaml
    with open(opts.config, "r") as stream:
        config = yaml.safe_load(stream)
    from cta_gan_amd import _lib, nets
    from cta_gan_amd.infer import SeriesTranslator, aspect_rows, view_angles
    from Model.HdGan import Generator
    _lib.load()
    mode = opts.dtype or DEFAULT_DTYPE
    nets.set_default_compute_dtype({"fp32": torch.float32, "bf16": torch.bfloat16}.get(mode, mode))
    print("compute mode: %s%s" % (nets.compute_mode(), "" if opts.dtype else " (default; --dtype fp32 is the reference's own arithmetic)"),
          flush=True)
    volume = np.load(opts.input)
    if volume.dtype != np.int16 or volume.ndim != 3:
        raise SystemExit("--input: an int16 [N, H, W] array expected, got %s %s" % (volume.dtype, volume.shape))
    device = torch.device("cuda", torch.cuda.current_device())
    generator = Generator(config["input_nc"], config["output_nc"]).to(device)
    generator.load_state_dict(torch.load(opts.weights, map_location=device))
    vr_lut = vr_options = None
    if opts.vr_dir is not None:      # the table is made here, corrected for the oversampling, so that render.npz can record it
        from cta_gan_amd.infer import TRANSFER_PRESETS, transfer_function
        vr_lut = transfer_function(TRANSFER_PRESETS[opts.vr_preset], opts.vr_oversample)
        vr_options = {"transfer": vr_lut, "wc": opts.vr_wc, "ww": opts.vr_ww, "sampling": opts.vr_sampling,
                      "oversample": opts.vr_oversample, "background": opts.vr_background}
    vr3d = vr3d_options = vr3d_lut = vr3d_light = None
    if opts.vr3d_dir is not None:      # the geometry, the table and the light are made here, so that render3d.npz can record them
        from cta_gan_amd.infer import TRANSFER_PRESETS, headlight, orbit_lines, transfer_function
        vr3d_lut = transfer_function(TRANSFER_PRESETS[opts.vr_preset], opts.vr_oversample)
        vr3d = orbit_lines(*volume.shape, view_angles(opts.vr_angles, opts.vr_span), axis=opts.vr3d_axis,
                           oversample=opts.vr_oversample, aspect=opts.aspect)
        vr3d_light = headlight(vr3d, opts.aspect) if opts.vr3d_shade else np.zeros((0, 3), dtype=np.int64)
        vr3d_options = {"transfer": vr3d_lut, "wc": opts.vr_wc, "ww": opts.vr_ww, "sampling": opts.vr3d_sampling,
                        "background": opts.vr_background, "aspect": opts.aspect,
                        "shading": {"ambient": opts.vr3d_ambient, "gmin": opts.vr3d_gmin, "light": "head"} if opts.vr3d_shade else None}
    reformat, reformat_angles = reformat_tables(opts)
    translate =SeriesTranslator(generator, batch=opts.batch, size=config.get("size"), wc=opts.wc, ww=opts.ww, hu=opts.hu,
                                 level=opts.level_dir is not None or opts.sub_level_dir is not None, device=device,
                                 subtract=opts.sub_output is not None, sub_median=not opts.sub_no_median, sub_floor=opts.sub_floor,
                                 sub_ct_range=(opts.sub_ct_min, opts.sub_ct_max), sub_window=(opts.sub_wc, opts.sub_ww),
                                 project_source=opts.mip_source,
                                 project=opts.mip_mode if opts.mip_dir is not None else None, slab=opts.slab,
                                 rotate=view_angles(opts.rot_angles, opts.rot_span) if opts.rot_dir is not None else None,
                                 rotate_mode=opts.mip_mode, rotate_sampling=opts.rot_sampling, rotate_oversample=opts.rot_oversample,
                                 slabs=opts.sts, depth=opts.depth, depth_cue=opts.depth_cue,
                                 render=view_angles(opts.vr_angles, opts.vr_span) if opts.vr_dir is not None else None,
                                 render_options=vr_options, reformat=reformat,
                                 reformat_options={"mode": opts.mip_mode, "sampling": opts.reformat_sampling} if reformat else None,
                                 render3d=None if vr3d is None else {"vr3d": vr3d}, render3d_options=vr3d_options,
                                 components=opts.cc, components_source=opts.cc_source, centreline=opts.cl)
    shown = "cued" if opts.depth_cue > 0 else "level"      # the plane the PNGs of the projections are written from
    out = translate(volume)
    rows = aspect_rows(volume.shape[0], opts.aspect)      # of the coronal / sagittal / rotating PNGs: --aspect repeats their rows
    np.save(opts.output, out["pix"])
    if opts.level_dir is not None:
        write_pngs(opts.level_dir, "%06d.png", out["level"])
    if opts.sub_output is not None:
        np.save(opts.sub_output, out["sub"])
        if opts.sub_level_dir is not None:
            write_pngs(opts.sub_level_dir, "%06d.png", out["sub_level"])
        print("wrote the subtraction volume to %s" % opts.sub_output, flush=True)
    if opts.cc_output is not None:
        from cta_gan_amd.infer import root_voxel
        ves = out["vessels"]
        np.save(opts.cc_output, ves["values"])
        if opts.cc_labels is not None:
            np.save(opts.cc_labels, ves["labels"])
        if opts.cc_level_dir is not None:
            write_pngs(opts.cc_level_dir, "%06d.png", ves["level"])
        roots = np.full((len(ves["top"]), 3), -1, dtype=np.int64)
        found = ves["top"][:, 0] >= 0
        if found.any():
            roots[found] = np.stack(root_voxel(ves["top"][found, 0], volume.shape[1], volume.shape[2]), axis=1)
        np.savez(os.path.join(os.path.dirname(os.path.abspath(opts.cc_output)), "components.npz"), top=ves["top"], stats=ves["stats"],
                 roots_zyx=roots)
        print("components: %d found, %d kept, %d voxels kept (wrote %s)" % (ves["stats"][1], ves["stats"][3], ves["stats"][4],
                                                                            opts.cc_output), flush=True)
    if opts.mip_dir is not None:
        proj = out["projections"]
        write_pngs(opts.mip_dir, "axial_%03d.png", proj["axial"][shown])
        for axis in ("coronal", "sagittal"):
            write_pngs(opts.mip_dir, axis + ".png", [proj[axis][shown]], rows)
        arrays = {axis: proj[axis]["values"] for axis in proj}
        if opts.depth:
            arrays.update({axis + "_depth": proj[axis]["depth"] for axis in proj})
        if opts.depth_cue > 0:
            arrays.update({axis + "_cued": proj[axis]["cued"] for axis in proj})
        np.savez(os.path.join(opts.mip_dir, "projections.npz"), **arrays)
        print("wrote the %s projections to %s" % (opts.mip_mode, opts.mip_dir), flush=True)
    if opts.rot_dir is not None:
        rot = out["rotation"]
        write_pngs(opts.rot_dir, "rot_%03d.png", rot[shown], rows)
        arrays = {"values": rot["values"], "level": rot["level"], "angles": rot["angles"]}
        if opts.depth:
            arrays["depth"] = rot["depth"]
        if opts.depth_cue > 0:
            arrays["cued"] = rot["cued"]
        np.savez(os.path.join(opts.rot_dir, "rotation.npz"), **arrays)
        print("wrote %d views of the %s projection to %s" % (len(rot["angles"]), opts.mip_mode, opts.rot_dir), flush=True)
    if opts.vr_dir is not None:
        ren = out["render"]
        write_pngs(opts.vr_dir, "vr_%03d.png", ren["rgb"], rows)      # uint8 [rows, D, 3]: mode "RGB"
        np.savez(os.path.join(opts.vr_dir, "render.npz"), rgb=ren["rgb"], opacity=ren["opacity"], depth=ren["depth"],
                 angles=ren["angles"], lut=vr_lut)
        print("wrote %d volume-rendered views (%s) to %s" % (len(ren["angles"]), opts.vr_preset, opts.vr_dir), flush=True)
    if opts.vr3d_dir is not None:
        ren = out["render3d"]["vr3d"]
        write_pngs(opts.vr3d_dir, "vr3d_%03d.png", ren["rgb"])      # mode "RGB"
        np.savez(os.path.join(opts.vr3d_dir, "render3d.npz"), rgb=ren["rgb"], opacity=ren["opacity"], depth=ren["depth"],
                 angles=np.array(view_angles(opts.vr_angles, opts.vr_span), dtype=np.float64), lut=vr3d_lut, lines=vr3d[0],
                 light=vr3d_light)
        print("wrote %d %s volume-rendered views (%s, %s sampling) to %s"
              % (len(ren["rgb"]), "shaded" if opts.vr3d_shade else "flat", opts.vr_preset, opts.vr3d_sampling, opts.vr3d_dir), flush=True)
    if opts.cl is not None:
        line = out["centreline"]
        if opts.cl_output is not None:
            np.save(opts.cl_output, line["points"][0])
        np.savez(os.path.join(os.path.dirname(os.path.abspath(opts.cl_output or opts.output)), "centreline.npz"), paths=line["paths"],
                 counts=line["counts"], stats=line["stats"], **{"points_%d" % e: p for e, p in enumerate(line["points"])})
        print("centreline: %d path(s) of %s voxels from %s%s" % (len(line["counts"]), ", ".join(str(int(c)) for c in line["counts"]),
              opts.cl_start, "" if opts.cl_output is None else " (wrote %s)" % opts.cl_output), flush=True)
    if opts.cl is not None and "lumen" in opts.cl:
        from cta_gan_amd.infer import lumen_profile, lumen_stenosis
        arrays = {}
        for e, tree in enumerate(out["centreline"]["lumen"]):
            prof = lumen_profile(tree, pixel_mm=opts.pixel_mm)
            arrays.update({"%s_%d" % (k, e): v for k, v in list(tree.items()) + list(prof.items())})
            try:
                g = lumen_stenosis(prof)
                print("lumen %d: %d of %d sections valid; narrowest at %.1f mm: diameter %.2f mm against a reference of %.2f mm: "
                      "%.0f %% diameter stenosis, %.0f %% by area" % (e, int(prof["valid"].sum()), len(prof["valid"]), prof["arc"][g["index"]],
                                                                     g["diameter"], g["reference_diameter"], g["percent_diameter"],
                                                                     g["percent_area"]), flush=True)
            except ValueError as err:
                print("lumen %d: %d of %d sections valid; no stenosis grade: %s" % (e, int(prof["valid"].sum()), len(prof["valid"]), err), flush=True)
        np.savez(opts.lumen_output, **arrays)
        print("wrote the lumen profile of %d centreline(s) to %s" % (len(out["centreline"]["lumen"]), opts.lumen_output), flush=True)
    if opts.cpr_traced:      # the curved reformat along the traced line of the first end (centreline.npz has every path)
        reformat_angles["cpr"] = opts.cl["cpr"]["angles"]
    for kind, where in (("mpr", opts.mpr_dir), ("tumble", opts.tumble_dir), ("cpr", opts.cpr_dir)):
        if where is None:
            continue
        traced = kind == "cpr" and opts.cpr_traced
        planes = out["centreline"]["cpr"][0] if traced else out["reformat"][kind]
        write_pngs(where, kind + "_%03d.png", planes["level"])
        arrays = {"values": planes["values"], "level": planes["level"]}
        if kind in reformat_angles:
            arrays["angles"] = np.array(reformat_angles[kind], dtype=np.float64)
        np.savez(os.path.join(where, "reformat.npz"), **arrays)
        print("wrote %d %s reformat(s)%s, %s sampling, to %s" % (len(planes["level"]), kind, " along the traced centreline" if traced else "",
                                                                opts.reformat_sampling, where), flush=True)
    if opts.sts_dir is not None:
        slabs = out["slabs"]
        for axis, d in slabs.items():
            write_pngs(opts.sts_dir, axis + "_%03d.png", d["level"], None if axis == "axial" else rows)
        np.savez(os.path.join(opts.sts_dir, "slabs.npz"), **{axis: d["values"] for axis, d in slabs.items()})
        print("wrote the %s thin slabs (%s) to %s" % (opts.mip_mode, ", ".join("%s: %d" % (a, len(d["values"]))
                                                                             for a, d in slabs.items()), opts.sts_dir), flush=True)
    print("wrote %s: %d slices of %d x %d%s" % (opts.output, volume.shape[0], volume.shape[1], volume.shape[2],
                                               "" if opts.level_dir is None else " (+ PNGs in %s)" % opts.level_dir), flush=True)


if __name__ == "__main__":
    main()
