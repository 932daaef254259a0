// IES photometric files, restated from the behaviour of IesData::parseIesFile (include/utility/util_ies.h:135-376).
#include "yafaray_ies.h"
#include <cmath>
#include <fstream>
#include <locale>
#include <sstream>

namespace yafies {

namespace {

struct Reader
{
	std::istringstream in;
	std::string name, *err;
	bool fail(const std::string &what) { *err = "IES file \"" + name + "\": " + what; return false; }
	// one `fin >> x` of the reference; a stream that cannot deliver it (the end of the file, or text that is no number) is a refusal here
	template<class T> bool read(T &x, const char *field)
	{
		if(in >> x) return true;
		return fail(std::string(in.eof() ? "the file ends before " : "cannot read ") + field);
	}
	bool skip(const char *field) { std::string s; return read(s, field); }
};

bool increasing(const std::vector<float> &m) { for(size_t i = 1; i < m.size(); ++i) if(!(m[i] > m[i - 1])) return false; return true; }

} // namespace

bool parse_text(const std::string &text, const std::string &name, Data &out, std::string &err)
{
	Reader r; r.name = name; r.err = &err;
	out = Data();
	if(text.size() < 7) return r.fail("too short to be an IES file (" + std::to_string(text.size()) + " bytes)");
	if(text.compare(0, 6, "IESNA:") != 0) return r.fail("wrong format, the first characters are not \"IESNA:\"");
	r.in.str(text);
	r.in.imbue(std::locale::classic());
	std::string tok;
	do { if(!(r.in >> tok)) return r.fail("no TILT= line before the end of the file"); } while(tok.find("TILT=") == std::string::npos);
	if(tok == "TILT=INCLUDE")
	{	// the lamp-to-luminaire geometry, the pair count, then the angles and the factors: skipped (:187-199)
		int pairs = 0;
		if(!r.skip("the tilt block's lamp geometry") || !r.read(pairs, "the tilt block's pair count")) return false;
		for(long long i = 0; i < 2ll * pairs; ++i) if(!r.skip("the tilt block's angles and factors")) return false;
	}
	float candela_mult = 0.f, w = 0.f, l = 0.f, h = 0.f;
	int n_vert = 0, n_hor = 0, type = 0;
	if(!r.skip("the number of lamps") || !r.skip("the lumens per lamp") || !r.read(candela_mult, "the candela multiplier")) return false;
	candela_mult *= 0.001;      // scaled and never applied (:225): the table is normalised by its own maximum
	(void)candela_mult;
	if(!r.read(n_vert, "the number of vertical angles") || !r.read(n_hor, "the number of horizontal angles") || !r.read(type, "the photometric type")) return false;
	if(!r.skip("the units type") || !r.read(w, "the opening's width") || !r.read(l, "the opening's length") || !r.read(h, "the opening's height")) return false;
	if(!r.skip("the ballast factor") || !r.skip("the ballast-lamp photometric factor") || !r.skip("the input watts")) return false;
	// sizes come from the counts only after this
	if(n_hor < 1 || n_vert < 2) return r.fail("needs at least 1 horizontal and 2 vertical angles, and claims " + std::to_string(n_hor) + " and " + std::to_string(n_vert));
	if(n_hor > kMaxAngles || n_vert > kMaxAngles)
		return r.fail("claims " + std::to_string(n_hor) + " horizontal and " + std::to_string(n_vert) + " vertical angles; more than " + std::to_string(kMaxAngles) + " of either are refused");
	const bool h_adjust = type == kTypeC && n_hor == 1;      // one horizontal angle: a second one at 180 with the same column (:336-340)
	const int n_hor_read = n_hor;
	if(h_adjust) ++n_hor;
	if(n_hor < 2) return r.fail("a single horizontal angle in a file that is not of type C: the lookup interpolates between two");
	if((long long)n_hor * (long long)n_vert > kMaxTable)
		return r.fail("claims a table of " + std::to_string((long long)n_hor * n_vert) + " values; more than " + std::to_string(kMaxTable) + " are refused");
	out.type = type; out.n_hor = n_hor; out.n_vert = n_vert;
	out.vert.resize((size_t)n_vert);
	float max_v = 0.f;
	for(int i = 0; i < n_vert; ++i)
	{
		if(!r.read(out.vert[(size_t)i], "the vertical angles")) return false;
		if(!std::isfinite(out.vert[(size_t)i])) return r.fail("a vertical angle that is not finite");
		if(max_v < out.vert[(size_t)i]) max_v = out.vert[(size_t)i];
	}
	if(out.vert[0] > 0.f)
	{	// a map that starts above 0 is moved down to 0 (:315-326)
		const float minus = out.vert[0];
		max_v -= minus;
		for(float &v : out.vert) v -= minus;
	}
	out.max_v_angle = (float)((double)max_v * 0.01745329251994329576922);      // DEG_TO_RAD, a double constant
	out.hor.resize((size_t)n_hor);
	for(int i = 0; i < n_hor_read; ++i)
	{
		if(!r.read(out.hor[(size_t)i], "the horizontal angles")) return false;
		if(!std::isfinite(out.hor[(size_t)i])) return r.fail("a horizontal angle that is not finite");
	}
	if(h_adjust) out.hor[1] = 180.f;
	// the lookup divides by the step between neighbours (:120-121)
	if(!increasing(out.vert)) return r.fail("the vertical angles are not strictly increasing");
	if(!increasing(out.hor)) return r.fail("the horizontal angles are not strictly increasing");
	out.table.resize((size_t)n_hor * (size_t)n_vert);
	float max_rad = 0.f;
	for(int i = 0; i < n_hor_read; ++i)
		for(int j = 0; j < n_vert; ++j)
		{
			float &v = out.table[(size_t)i * (size_t)n_vert + (size_t)j];
			if(!r.read(v, "the candela values")) return false;
			if(!std::isfinite(v)) return r.fail("a candela value that is not finite");
			if(max_rad < v) max_rad = v;
		}
	if(h_adjust) for(int j = 0; j < n_vert; ++j) out.table[(size_t)n_vert + (size_t)j] = out.table[(size_t)j];
	if(!(max_rad > 0.f)) return r.fail("no candela value above zero: nothing to normalise the table by");
	out.max_rad = 1.f / max_rad;
	if(!std::isfinite(out.max_rad)) return r.fail("the largest candela value is too small to normalise the table by");
	return true;
}

bool parse_file(const std::string &path, Data &out, std::string &err)
{
	std::ifstream f(path.c_str(), std::ios::in | std::ios::binary);
	if(!f) { err = "IES file \"" + path + "\": cannot open it"; return false; }
	std::ostringstream ss;
	ss << f.rdbuf();
	return parse_text(ss.str(), path, out, err);
}

} // namespace yafies
