// pbrt_params.h — the tokens and typed parameter lists of a .pbrt file (the loader's input side).
//
// Tokenizer of src/core/parser.cpp:150-255, number parsing of parser.cpp:258-300, and the parameter lookups the loader needs of
// ParamSet (src/core/paramset.cpp). Header-only.
#pragma once
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace iile {

struct Token {
    enum Kind { Word, String, LBracket, RBracket, End, Error } kind = End;
    std::string text;  // Error: the tokenizer's message ("premature EOF", "unterminated string")
};

class Lexer {
  public:
    bool open(const std::string &path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) return false;
        std::stringstream ss;
        ss << f.rdbuf();
        buf_ = ss.str();
        pos_ = 0;
        return true;
    }
    // parser.cpp:150-255: whitespace, '#' comments, quoted strings, brackets,
    // everything else runs to the next delimiter.
    Token next() {
        Token t;
        while (pos_ < buf_.size()) {
            char ch = buf_[pos_];
            if (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r') {
                ++pos_;
            } else if (ch == '#') {
                while (pos_ < buf_.size() && buf_[pos_] != '\n' && buf_[pos_] != '\r') ++pos_;
            } else
                break;
        }
        if (pos_ >= buf_.size()) return t;
        char ch = buf_[pos_];
        if (ch == '"') {
            // scan to the closing quote (parser.cpp:196-232): a newline ends the string in error,
            // a backslash takes the next character with it (decodeEscaped, parser.cpp:67-93)
            t.kind = Token::String;
            ++pos_;
            for (;;) {
                if (pos_ >= buf_.size()) {
                    t.kind = Token::Error;
                    t.text = "premature EOF";
                    return t;
                }
                char c = buf_[pos_++];
                if (c == '"') break;
                if (c == '\n') {
                    t.kind = Token::Error;
                    t.text = "unterminated string";
                    return t;
                }
                if (c == '\\') {
                    if (pos_ >= buf_.size()) {
                        t.kind = Token::Error;
                        t.text = "premature EOF";
                        return t;
                    }
                    const char e = buf_[pos_++];
                    switch (e) {
                    case 'b': c = '\b'; break;
                    case 'f': c = '\f'; break;
                    case 'n': c = '\n'; break;
                    case 'r': c = '\r'; break;
                    case 't': c = '\t'; break;
                    case '\\': c = '\\'; break;
                    case '\'': c = '\''; break;
                    case '"': c = '"'; break;
                    default:
                        t.kind = Token::Error;
                        t.text = std::string("unexpected escaped character \"") + e + "\"";
                        return t;
                    }
                }
                t.text.push_back(c);
            }
        } else if (ch == '[') {
            t.kind = Token::LBracket;
            ++pos_;
        } else if (ch == ']') {
            t.kind = Token::RBracket;
            ++pos_;
        } else {
            size_t s = pos_;
            while (pos_ < buf_.size()) {
                char c = buf_[pos_];
                if (c == ' ' || c == '\n' || c == '\t' || c == '\r' || c == '"' || c == '[' || c == ']')
                    break;
                ++pos_;
            }
            t.kind = Token::Word;
            t.text = buf_.substr(s, pos_ - s);
        }
        return t;
    }

  private:
    std::string buf_;
    size_t pos_ = 0;
};

// parser.cpp:258-300: all-digit tokens go through strtol, everything else
// through strtof; the value travels as double and is cast at the use site.
inline bool parse_number(const std::string &s, double *out) {
    if (s.size() == 1) {
        if (!(s[0] >= '0' && s[0] <= '9')) return false;
        *out = s[0] - '0';
        return true;
    }
    bool is_int = true;
    for (char c : s)
        if (!(c >= '0' && c <= '9')) is_int = false;
    char *end = nullptr;
    double v;
    if (is_int)
        v = double(strtol(s.c_str(), &end, 10));
    else
        v = strtof(s.c_str(), &end);
    if (v == 0 && end == s.c_str()) return false;
    *out = v;
    return true;
}

struct Param {
    std::string type, name;
    std::vector<double> nums;
    std::vector<std::string> strs;
};
struct ParamSet {
    std::vector<Param> params;
    const Param *find(const std::string &name) const {
        for (const Param &p : params)
            if (p.name == name) return &p;
        return nullptr;
    }
    float one_float(const std::string &name, float def) const {
        const Param *p = find(name);
        return (p && p->type == "float" && p->nums.size() == 1) ? float(p->nums[0]) : def;
    }
    int one_int(const std::string &name, int def) const {
        const Param *p = find(name);
        return (p && p->type == "integer" && p->nums.size() == 1) ? int(p->nums[0]) : def;
    }
    bool one_bool(const std::string &name, bool def) const {
        const Param *p = find(name);
        if (!p || p->type != "bool" || p->strs.size() != 1) return def;
        return p->strs[0] == "true";
    }
    std::string one_string(const std::string &name, const std::string &def) const {
        const Param *p = find(name);
        return (p && p->type == "string" && p->strs.size() == 1) ? p->strs[0] : def;
    }
    bool rgb(const std::string &name, float out[3]) const {
        const Param *p = find(name);
        if (!p || (p->type != "color" && p->type != "rgb") || p->nums.size() != 3) return false;
        for (int i = 0; i < 3; ++i) out[i] = float(p->nums[i]);
        return true;
    }
};

}  // namespace iile
