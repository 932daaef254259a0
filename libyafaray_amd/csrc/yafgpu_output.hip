// The output stage on the device: a film [h][w][5] (r, g, b, a, weight) becomes the packed pixels of an image file, one pixel per lane.
//
// Per pixel, in the order of ImageFilm::flush for the combined pass (imagefilm.cc:737-772), which is also what the host's deliver_to /
// to_output_space (yafaray_c_api.cpp) hand to a ColorOutput's putPixel:
//   Pixel::normalized  (colour and alpha times (float)(1.0 / (double)weight), zero where the weight is 0)
//   clampRgb0          (std::max(0.f, c))
//   Rgb::colorSpaceFromLinearRgb (color.h:388-411): sRGB through fPow__, XYZ by the D65 matrix, RawManualGamma through fPow__(c, 1 / gamma)
//   alpha clamped to [0, 1]
// and then one of three packings:
//   YAFGPU_IMAGE_FLOAT  the four floats as they are (one 128-bit store)
//   YAFGPU_IMAGE_RGBA8  clampRgba01, then (uint8_t)(c * 255.f): a truncation, as TgaPixelRgba::operator= (imagehandler_util_tga.h) and
//                       PngHandler::saveToFile (imagehandler_png.cc:138-141) do it; bytes r g b a; without alpha the alpha byte is 255
//   YAFGPU_IMAGE_RGBE   RgbePixel::operator=(const Rgb &) (imagehandler_util_hdr.h:52-71): v = max(r, g, b); below 1e-32 four zero bytes;
//                       else v = (float)(frexp(v, &e) * 255.9999 / v) with the product and the quotient in double, bytes (uint8_t)(c * v)
//                       and (uint8_t)(e + 128)
// The unit is built with the flags of the other units (no contraction, IEEE divide), so that every expression rounds as the host's does.
//
// Values the reference's casts leave undefined are defined here: a NaN channel packs to the byte 0, and a pixel whose largest colour
// channel is not finite packs to four zero bytes in RGBE.  The float format hands non-finite values on as they are.
#include "../../include/yafgpu.h"
#include "yafgpu_math.h"

#include <string>

extern "C" void yafgpu_internal_set_error(const char *msg);      // the device unit's yafgpu_last_error() text

namespace yafgpu {
namespace {

constexpr int kOutBlock = 256;

struct OutArgs
{
	uint32_t w, h;               // the film: the render window
	uint32_t img_w, bx, by;      // row length of the image and where the window starts in it
	int32_t color_space;         // 0 sRGB, 1 XYZ, 2 LinearRGB, 3 RawManualGamma
	float inv_gamma;             // RawManualGamma: 1 / gamma, worked out by the host as to_output_space does; 1 = leave alone
	int32_t alpha;               // RGBA8: 0 = the alpha byte is 255
};

YG_DEV void output_space(const OutArgs &a, float c[4])
{
	if(a.color_space == 0)
	{
		for(int k = 0; k < 3; ++k) c[k] = (c[k] <= 0.0031308f) ? (c[k] * 12.92f) : ((1.055f * f_pow(c[k], 0.416667f)) - 0.055f);
	}
	else if(a.color_space == 1)
	{
		const float o0 = c[0], o1 = c[1], o2 = c[2];
		c[0] = 0.412400f * o0 + 0.357600f * o1 + 0.180500f * o2;
		c[1] = 0.212600f * o0 + 0.715200f * o1 + 0.072200f * o2;
		c[2] = 0.019300f * o0 + 0.119200f * o1 + 0.950500f * o2;
	}
	else if(a.color_space == 3 && a.inv_gamma != 1.f)
	{
		for(int k = 0; k < 3; ++k) c[k] = f_pow(c[k], a.inv_gamma);
	}
	if(c[3] < 0.f) c[3] = 0.f; else if(c[3] > 1.f) c[3] = 1.f;
}

YG_DEV uint32_t byte_of(float c)       // clampRgba01's branch, then (uint8_t)(c * 255.f); NaN -> 0
{
	if(c < 0.f) c = 0.f; else if(c > 1.f) c = 1.f;
	return c == c ? (uint32_t)(c * 255.f) : 0u;
}

YG_DEV uint32_t pack_rgbe(const float c[4])
{
	const float v = smax(c[0], smax(c[1], c[2]));      // Rgb::maximum
	if((double)v < 1e-32) return 0u;
	const uint32_t bits = (uint32_t)__float_as_int(v);
	if((bits & 0x7f800000u) == 0x7f800000u) return 0u;      // not finite: undefined in the reference, zero here
	// frexp of a normal float: the mantissa in [0.5, 1) and the exponent that goes with it (v >= 1e-32 is normal)
	const int e = (int)((bits >> 23) & 0xffu) - 126;
	const float m = __int_as_float((int)((bits & 0x807fffffu) | (126u << 23)));
	const float s = (float)((double)m * 255.9999 / (double)v);
	// (c <= v, so c * s stays below 256; the colours are clamped at zero before they get here)
	const uint32_t r = (uint32_t)(c[0] * s) & 0xffu, g = (uint32_t)(c[1] * s) & 0xffu, b = (uint32_t)(c[2] * s) & 0xffu;
	return r | (g << 8) | (b << 16) | (((uint32_t)(e + 128) & 0xffu) << 24);
}

template<int kFormat>
__global__ __launch_bounds__(kOutBlock) void film_to_image_kernel(const float *__restrict__ film, OutArgs a, void *__restrict__ out)
{
	const uint64_t n = (uint64_t)a.w * (uint64_t)a.h;
	const uint64_t i = (uint64_t)blockIdx.x * (uint64_t)kOutBlock + (uint64_t)threadIdx.x;
	if(i >= n) return;
	const uint32_t y = (uint32_t)(i / a.w), x = (uint32_t)(i - (uint64_t)y * a.w);
	const float *px = film + 5u * i;
	float c[4] = {0.f, 0.f, 0.f, 0.f};
	const float weight = px[4];
	if(weight != 0.f)
	{
		const float f = (float)(1.0 / (double)weight);       // Pixel::normalized, Rgba / float (color.h:310-314)
		for(int k = 0; k < 4; ++k) c[k] = px[k] * f;
	}
	for(int k = 0; k < 3; ++k) c[k] = smax(0.f, c[k]);       // clampRgb0
	output_space(a, c);
	const uint64_t o = (uint64_t)(y + a.by) * (uint64_t)a.img_w + (uint64_t)(x + a.bx);
	if(kFormat == YAFGPU_IMAGE_FLOAT)
	{
		float4 v; v.x = c[0]; v.y = c[1]; v.z = c[2]; v.w = c[3];
		((float4 *)out)[o] = v;
	}
	else if(kFormat == YAFGPU_IMAGE_RGBA8)
	{
		const uint32_t al = a.alpha ? byte_of(c[3]) : 255u;
		((uint32_t *)out)[o] = byte_of(c[0]) | (byte_of(c[1]) << 8) | (byte_of(c[2]) << 16) | (al << 24);
	}
	else ((uint32_t *)out)[o] = pack_rgbe(c);
}

int out_fail(int code, const std::string &msg) { yafgpu_internal_set_error(msg.c_str()); return code; }

} // namespace
} // namespace yafgpu

using namespace yafgpu;

extern "C" uint64_t yafgpu_image_bytes(int32_t format, int32_t width, int32_t height)
{
	if(width <= 0 || height <= 0 || format < YAFGPU_IMAGE_FLOAT || format > YAFGPU_IMAGE_RGBE) return 0;
	return (uint64_t)width * (uint64_t)height * (format == YAFGPU_IMAGE_FLOAT ? 16u : 4u);
}

extern "C" int yafgpu_film_to_image(const float *d_film, const yafgpu_image_desc *desc, void *d_image, void *stream_)
{
	if(!d_film || !desc || !d_image) return out_fail(-1, "film to image: null argument");
	const yafgpu_image_desc &d = *desc;
	if(d.format < YAFGPU_IMAGE_FLOAT || d.format > YAFGPU_IMAGE_RGBE) return out_fail(-2, "film to image: unknown pixel format " + std::to_string(d.format));
	if(d.color_space < 0 || d.color_space > 3) return out_fail(-2, "film to image: unknown colour space " + std::to_string(d.color_space));
	// every index the kernel forms is checked here, in 64 bits, before anything is launched
	constexpr int64_t kMaxPixels = (int64_t)1 << 28;
	if(d.width <= 0 || d.height <= 0 || (int64_t)d.width * (int64_t)d.height > kMaxPixels) return out_fail(-10, "film to image: film size out of range");
	if(d.image_width <= 0 || d.image_height <= 0 || (int64_t)d.image_width * (int64_t)d.image_height > kMaxPixels) return out_fail(-10, "film to image: image size out of range");
	if(d.border_x < 0 || d.border_y < 0 || (int64_t)d.border_x + d.width > d.image_width || (int64_t)d.border_y + d.height > d.image_height)
		return out_fail(-11, "film to image: a window of " + std::to_string(d.width) + " x " + std::to_string(d.height) + " at (" + std::to_string(d.border_x) + ", " +
		                     std::to_string(d.border_y) + ") does not fit an image of " + std::to_string(d.image_width) + " x " + std::to_string(d.image_height));
	const size_t align = d.format == YAFGPU_IMAGE_FLOAT ? 16 : 4;
	if(((uintptr_t)d_image % align) != 0 || ((uintptr_t)d_film % 4) != 0) return out_fail(-12, "film to image: misaligned device pointer");
	hipStream_t stream = (hipStream_t)stream_;
	hipError_t e = hipSuccess;
	// pixels outside the render window stay zero
	if(d.image_width != d.width || d.image_height != d.height)
		if((e = hipMemsetAsync(d_image, 0, (size_t)yafgpu_image_bytes(d.format, d.image_width, d.image_height), stream)) != hipSuccess)
			return out_fail(-100, std::string("film to image: ") + hipGetErrorString(e));
	OutArgs a{};
	a.w = (uint32_t)d.width; a.h = (uint32_t)d.height; a.img_w = (uint32_t)d.image_width; a.bx = (uint32_t)d.border_x; a.by = (uint32_t)d.border_y;
	a.color_space = d.color_space; a.alpha = d.alpha ? 1 : 0;
	a.inv_gamma = 1.f;
	if(d.color_space == 3 && d.gamma != 1.f) { float gamma = d.gamma; if(gamma <= 0.f) gamma = 1.0e-2f; a.inv_gamma = 1.f / gamma; }     // Rgb::gammaAdjust(1 / gamma)
	const uint64_t n = (uint64_t)d.width * (uint64_t)d.height;
	const dim3 grid((uint32_t)((n + kOutBlock - 1) / kOutBlock)), block(kOutBlock);
	switch(d.format)
	{
		case YAFGPU_IMAGE_FLOAT: hipLaunchKernelGGL(film_to_image_kernel<YAFGPU_IMAGE_FLOAT>, grid, block, 0, stream, d_film, a, d_image); break;
		case YAFGPU_IMAGE_RGBA8: hipLaunchKernelGGL(film_to_image_kernel<YAFGPU_IMAGE_RGBA8>, grid, block, 0, stream, d_film, a, d_image); break;
		default: hipLaunchKernelGGL(film_to_image_kernel<YAFGPU_IMAGE_RGBE>, grid, block, 0, stream, d_film, a, d_image); break;
	}
	if((e = hipGetLastError()) != hipSuccess) return out_fail(-100, std::string("film to image: ") + hipGetErrorString(e));
	return 0;
}
