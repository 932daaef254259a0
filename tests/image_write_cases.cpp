// TEST SUPPORT: the image file encoders (csrc/yafaray_image.cpp) as a program of their own, for a run under AddressSanitizer + UBSan
// on the CPU (tests/test_image_output_host.py builds and runs it; nothing is loaded into Python).
//   image_write_cases <directory>
// Every file <name>_<w>x<h>.px of the directory holds w * h packed pixels, four bytes each.  Each is written as <name>_<w>x<h>.tga and
// .png without alpha, _a.tga and _a.png with alpha, and .hdr, beside it: the test compares them with the files the library wrote for
// the same pixels.  Then the refusals: sizes below 1, sizes no format holds, more pixels than an image may have (with a one-pixel buffer:
// an encoder that allocated or read before it checked would be caught), a directory that does not exist.  The packers run over every
// pixel's bytes taken as floats' worth of values, non-finite ones among them.
// Prints "wrote N, refused M, failures 0"; the exit status is the number of failures.
#include "yafaray_image.h"

#include <dirent.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

static int failures = 0;
static void expect(bool ok, const std::string &what)
{
	if(!ok) { ++failures; std::printf("FAILED: %s\n", what.c_str()); }
}

int main(int argc, char **argv)
{
	if(argc != 2) { std::fprintf(stderr, "usage: image_write_cases <directory>\n"); return 100; }
	const std::string dir = argv[1];
	int wrote = 0, refused = 0;
	std::vector<std::string> names;
	if(DIR *d = ::opendir(dir.c_str()))
	{
		while(const dirent *e = ::readdir(d))
		{
			const std::string n = e->d_name;
			if(n.size() > 3 && n.compare(n.size() - 3, 3, ".px") == 0) names.push_back(n.substr(0, n.size() - 3));
		}
		::closedir(d);
	}
	expect(!names.empty(), "no .px files in " + dir);
	for(const std::string &name : names)
	{
		const size_t us = name.rfind('_'), x = name.rfind('x');
		if(us == std::string::npos || x == std::string::npos || x < us) { expect(false, "file name " + name); continue; }
		const int w = std::atoi(name.substr(us + 1, x - us - 1).c_str()), h = std::atoi(name.substr(x + 1).c_str());
		std::vector<uint8_t> px((size_t)w * (size_t)h * 4);
		FILE *fp = std::fopen((dir + "/" + name + ".px").c_str(), "rb");
		const bool read = fp && std::fread(px.data(), 1, px.size(), fp) == px.size();
		if(fp) std::fclose(fp);
		expect(read, "reading " + name);
		if(!read) continue;
		std::string err;
		const std::string base = dir + "/" + name;
		expect(yafimg::write_tga(base + ".tga", w, h, false, px.data(), err), "tga " + name + ": " + err);
		expect(yafimg::write_tga(base + "_a.tga", w, h, true, px.data(), err), "tga with alpha " + name + ": " + err);
		expect(yafimg::write_png(base + ".png", w, h, false, px.data(), err), "png " + name + ": " + err);
		expect(yafimg::write_png(base + "_a.png", w, h, true, px.data(), err), "png with alpha " + name + ": " + err);
		expect(yafimg::write_hdr(base + ".hdr", w, h, px.data(), err), "hdr " + name + ": " + err);
		wrote += 5;
	}
	// refusals: each with a cause, none touching more than the one pixel it is given
	{
		const uint8_t one[4] = {1, 2, 3, 4};
		const int big = std::numeric_limits<int>::max();
		const int sizes[][2] = {{0, 1}, {1, 0}, {-1, 4}, {4, -7}, {65536, 65536}, {big, big}, {big, 1}, {8193, 8193}};
		for(const auto &s : sizes)
		{
			std::string err;
			const bool tga = yafimg::write_tga(dir + "/refused.tga", s[0], s[1], true, one, err);
			expect(!tga && !err.empty(), "tga accepted " + std::to_string(s[0]) + " x " + std::to_string(s[1]));
			err.clear();
			const bool png = yafimg::write_png(dir + "/refused.png", s[0], s[1], true, one, err);
			expect(!png && !err.empty(), "png accepted " + std::to_string(s[0]) + " x " + std::to_string(s[1]));
			err.clear();
			const bool hdr = yafimg::write_hdr(dir + "/refused.hdr", s[0], s[1], one, err);
			expect(!hdr && !err.empty(), "hdr accepted " + std::to_string(s[0]) + " x " + std::to_string(s[1]));
			refused += 3;
		}
		std::string err;
		expect(!yafimg::write_tga(dir + "/refused.tga", 70000, 1, false, one, err) && !err.empty(), "tga accepted a side of 70000"); ++refused;
		err.clear();
		expect(!yafimg::write_png(dir + "/no/such/directory/a.png", 1, 1, false, one, err) && err.find("cannot be created") != std::string::npos, "png into a missing directory: " + err); ++refused;
		err.clear();
		expect(!yafimg::write_hdr(dir + "/no/such/directory/a.hdr", 1, 1, one, err) && err.find("cannot be created") != std::string::npos, "hdr into a missing directory: " + err); ++refused;
		err.clear();
		expect(!yafimg::write_tga(dir + "/a.tga", 1, 1, false, nullptr, err) && !err.empty(), "tga accepted null pixels"); ++refused;
	}
	// the packers over ordinary and extreme values: every cast they make must be defined
	{
		const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
		const float vals[] = {0.f, -1.f, 1e-33f, 1e-32f, 0.5f, 1.f, 255.f / 256.f, 2.f, 1e30f, 3.4e38f, inf, -inf, nan};
		unsigned sum = 0;
		for(float r : vals) for(float g : vals) for(float a : vals)
		{
			const float c[4] = {r, g, 0.25f, a};
			uint8_t o[4];
			yafimg::pack_rgba8(c, true, o); sum += o[0] + o[1] + o[2] + o[3];
			yafimg::pack_rgbe(c, o); sum += o[0] + o[1] + o[2] + o[3];
		}
		expect(sum != 0, "packers");
	}
	std::printf("wrote %d, refused %d, failures %d\n", wrote, refused, failures);
	return failures;
}
