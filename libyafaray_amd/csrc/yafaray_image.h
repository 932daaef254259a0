// Host-side image textures: see yafaray_image.cpp
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace yafimg {

enum { kSrgb = 0, kXyz = 1, kLinearRgb = 2, kRawManualGamma = 3 };          // ColorSpace, include/common/color.h
enum { kOptNone = 0, kOptOptimized = 1, kOptCompressed = 2 };                 // TextureOptimization

struct Image
{
	// in: how the file's colours are to be read and kept (ImageHandler::setColorSpace / setTextureOptimization / setGrayScaleSetting)
	int color_space = kRawManualGamma; float gamma = 1.f; int optimization = kOptOptimized; bool grayscale = false;
	// out
	int width = 0, height = 0, channels = 0; bool has_alpha = false;
	std::vector<float> texels;         // height * width * 4: what ImageHandler::getPixel(x, y) returns, row y = the handler's row y
};

// decodes `path` by its extension (tga, hdr, png); false + err for anything else or a damaged file
bool load(const std::string &path, Image &img, std::string &err);

// ---- image file encoders (TgaHandler / HdrHandler / PngHandler ::saveToFile).  The pixels come in packed, as the device's output stage
// (yafgpu_output.hip) or the two packers below make them: rgba8 = w * h * 4 bytes r g b a, rgbe = w * h * 4 bytes r g b e, rows from the
// top.  All refuse a size below 1, a size the format cannot hold and more than 2^26 pixels before anything is allocated, and return
// false + err (the path and the cause) for a file that cannot be created or written in full.  None throws.
//   write_tga  imagehandler_tga.cc:47-136: the 18-byte TgaHeader (uncompressed true colour, 24 bits or 32 with alpha, top-left origin),
//              the id "Image rendered with YafaRay", pixels as B G R [A], the 26-byte TgaFooter with the TRUEVISION-XFILE signature
//   write_hdr  imagehandler_hdr.cc:392-533: writeHeader's text, then per scanline the start signature 2 2 w>>8 w&255 and four channel
//              blocks with writeScanline's run logic (restated so that it never reads past the scanline).  A width outside 8 .. 32767 cannot
//              carry that signature: such scanlines are written flat, four bytes a pixel
//   write_png  8-bit RGB, or RGBA with alpha, non-interlaced, every row with filter 0, one zlib stream in one IDAT chunk.  The bytes are not
//              libpng's; the decoded pixels are
bool write_tga(const std::string &path, int w, int h, bool alpha, const uint8_t *rgba8, std::string &err);
bool write_hdr(const std::string &path, int w, int h, const uint8_t *rgbe, std::string &err);
bool write_png(const std::string &path, int w, int h, bool alpha, const uint8_t *rgba8, std::string &err);
// The two packers on the host, for pixels a caller delivers one by one: clampRgba01 and (uint8_t)(c * 255.f) (TgaPixelRgba::operator=,
// PngHandler::saveToFile:138-141; without alpha the alpha byte is 255), and RgbePixel::operator=(const Rgb &)
// (imagehandler_util_hdr.h:52-71).  A NaN channel gives the byte 0 and a largest channel that is not finite four zero bytes, as on the device.
void pack_rgba8(const float c[4], bool alpha, uint8_t out[4]);
void pack_rgbe(const float c[4], uint8_t out[4]);

// ---- film files (ImageFilm::imageFilmSave / imageFilmLoad, imagefilm.cc:1560-1657, :1340-1465), little-endian:
//   "YAF_FILMv1" 0x00 | the eleven 32-bit words of FilmHeader | (n_passes + n_aux) x h x w x { float r, g, b, a, weight }
struct FilmHeader
{
	uint32_t computer_node = 0, base_sampling_offset = 0, sampling_offset = 0;
	int32_t w = 0, h = 0, cx0 = 0, cx1 = 0, cy0 = 0, cy1 = 0, n_passes = 1, n_aux = 0;
};
constexpr uint64_t kFilmHeaderBytes = 11 + 44;      // the string with its terminator, the header words
// writes the combined pass alone: n_passes = 1 and n_aux = 0 go into the file whatever hdr says; film = h * w * 5 floats
bool write_film(const std::string &path, const FilmHeader &hdr, const float *film_hw5, std::string &err);
// Reads the header and, with film_hw5, pass 0 of the payload into it (n_floats must be h * w * 5); further passes are skipped.
// False + err, with hdr and the buffer untouched, for: a wrong or unterminated magic, a negative count, no pass at all, a length
// that is not exactly what the header promises (checked in 64 bits before anything is read or allocated).  Never throws.
bool read_film(const std::string &path, FilmHeader &hdr, float *film_hw5, uint64_t n_floats, std::string &err);

} // namespace yafimg
