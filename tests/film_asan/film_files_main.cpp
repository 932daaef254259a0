// TEST SUPPORT: the film-file reader and writer (yafimg::read_film / write_film, csrc/yafaray_image.cpp) over a directory of crafted
// files, as a program of its own so that it can run under AddressSanitizer + UBSan without anything being loaded into Python.
//
//   film_files_main <directory>
// Every "ok_*.film" in the directory must read, its pass 0 must survive a round trip through the writer, and a file that holds one
// pass alone must be rewritten byte for byte.  Every "bad_*.film" must be refused with a cause, by the header-only call and by the call
// with a buffer, and the buffer must come back untouched.  Exit status 0 when all of that holds.
#include "../../libyafaray_amd/csrc/yafaray_image.h"

#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static std::vector<unsigned char> bytes_of(const std::string &path)
{
	std::vector<unsigned char> out;
	if(FILE *f = std::fopen(path.c_str(), "rb"))
	{
		unsigned char buf[4096];
		size_t n;
		while((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
		std::fclose(f);
	}
	return out;
}

int main(int argc, char **argv)
{
	if(argc != 2) { std::fprintf(stderr, "usage: %s <directory>\n", argv[0]); return 2; }
	const std::string dir = argv[1];
	std::vector<std::string> names;
	if(DIR *d = ::opendir(dir.c_str()))
	{
		while(const dirent *e = ::readdir(d)) names.push_back(e->d_name);
		::closedir(d);
	}
	std::sort(names.begin(), names.end());
	int n_ok = 0, n_bad = 0, failures = 0;
	for(const std::string &name : names)
	{
		const bool ok_file = name.compare(0, 3, "ok_") == 0, bad_file = name.compare(0, 4, "bad_") == 0;
		if(name.size() < 5 || name.compare(name.size() - 5, 5, ".film") != 0 || !(ok_file || bad_file)) continue;
		const std::string path = dir + "/" + name;
		yafimg::FilmHeader hdr;
		std::string err;
		if(bad_file)
		{
			++n_bad;
			const yafimg::FilmHeader before = hdr;
			const float mark = -12345.f;
			std::vector<float> buf(10, mark);      // the crafted films are 2 x 1
			bool refused = !yafimg::read_film(path, hdr, nullptr, 0, err) && !err.empty();
			err.clear();
			refused = refused && !yafimg::read_film(path, hdr, buf.data(), buf.size(), err) && !err.empty();
			const bool untouched = std::count(buf.begin(), buf.end(), mark) == (long)buf.size() && std::memcmp(&before, &hdr, sizeof hdr) == 0;
			if(!refused || !untouched) { ++failures; std::printf("FAIL %s: refused %d untouched %d\n", name.c_str(), (int)refused, (int)untouched); }
			continue;
		}
		++n_ok;
		if(!yafimg::read_film(path, hdr, nullptr, 0, err)) { ++failures; std::printf("FAIL %s: %s\n", name.c_str(), err.c_str()); continue; }
		std::vector<float> film((size_t)hdr.w * (size_t)hdr.h * 5);
		if(!yafimg::read_film(path, hdr, film.data(), film.size(), err)) { ++failures; std::printf("FAIL %s: %s\n", name.c_str(), err.c_str()); continue; }
		const std::string copy = path + ".rewritten";
		yafimg::FilmHeader hdr2;
		std::vector<float> film2(film.size());
		if(!yafimg::write_film(copy, hdr, film.data(), err) || !yafimg::read_film(copy, hdr2, film2.data(), film2.size(), err))
		{ ++failures; std::printf("FAIL %s (rewritten): %s\n", name.c_str(), err.c_str()); continue; }
		bool same = hdr2.n_passes == 1 && hdr2.n_aux == 0 && hdr2.w == hdr.w && hdr2.h == hdr.h && hdr2.sampling_offset == hdr.sampling_offset &&
		            (film.empty() || std::memcmp(film.data(), film2.data(), film.size() * sizeof(float)) == 0);
		if(hdr.n_passes == 1 && hdr.n_aux == 0) same = same && bytes_of(path) == bytes_of(copy);
		if(!same) { ++failures; std::printf("FAIL %s: the rewritten file differs\n", name.c_str()); }
	}
	std::printf("read %d, refused %d, failures %d\n", n_ok, n_bad - failures, failures);
	return failures == 0 && n_ok + n_bad > 0 ? 0 : 1;
}
