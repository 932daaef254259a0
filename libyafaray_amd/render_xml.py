"""Render a YafaRay scene XML to an image file:

    python -m libyafaray_amd.render_xml scene.xml -o out.png [-f tga|hdr|png] [--alpha]

The scene is loaded by the C++ XML loader, rendered on the GPU and written from the device film by an image output (createImageHandler +
ImageOutput + render, include/yafaray_c_api.h): the file's size is the render's width x height, its colours are in the scene's color_space.
"""
import argparse
import os
import sys

from .interface import Interface, YafaRayError

FORMATS = {"tga": "tga", "hdr": "hdr", "pic": "hdr", "png": "png"}


def render_xml(scene, out, fmt=None, alpha=False):
    """-> the Interface after the render (its film and statistics are there to be read); raises YafaRayError with the cause"""
    if fmt is None:
        fmt = os.path.splitext(os.fspath(out))[1].lstrip(".").lower()
    if fmt not in FORMATS:
        raise YafaRayError(f"image format \"{fmt}\": tga, hdr and png files are written (name one with -f, or by the output's extension)")
    yi = Interface(strict=True)
    yi.loadXml(os.fspath(scene))
    # the handler takes its size from the render's own width and height, which the loader left in the parameters
    yi.paramsSetString("type", FORMATS[fmt])
    yi.paramsSetBool("alpha_channel", bool(alpha))
    handler = yi.createImageHandler("render_xml_output")
    image = yi.createImageOutput(handler, out)
    try:
        yi.render(output=image)
    finally:
        image.close()
    return yi


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m libyafaray_amd.render_xml", description="render a YafaRay scene XML to a TGA, HDR or PNG file")
    ap.add_argument("scene", help="the scene XML")
    ap.add_argument("-o", "--output", required=True, help="the image file to write")
    ap.add_argument("-f", "--format", choices=sorted(FORMATS), default=None, help="the file format (default: by the output's extension)")
    ap.add_argument("--alpha", action="store_true", help="write the alpha channel (tga and png)")
    args = ap.parse_args(argv)
    try:
        yi = render_xml(args.scene, args.output, args.format, args.alpha)
    except YafaRayError as e:
        print(f"render_xml: {e}", file=sys.stderr)
        return 1
    st = yi.getRenderStats()
    print(f"{args.output}: {st.camera_samples} camera samples, {st.rays_closest + st.rays_shadow} rays, {st.render_seconds:.3f} s on the device")
    return 0


if __name__ == "__main__":
    sys.exit(main())
