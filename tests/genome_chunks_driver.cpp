// genome_chunks_driver.cpp -- host/genome_chunks.hpp under AddressSanitizer and UBSan (tests/test_build_parse_cpu.py builds and runs it):
// the cut rule on buffers of exactly the bytes there are, and the letters of a short record against a restatement of the record rules.
#include "../ganon_amd/host/genome_chunks.hpp"

#include <cstdlib>
#include <iostream>
#include <memory>
#include <random>
#include <string>

namespace
{

int checks = 0;

void expect(bool ok, const std::string& what)
{
    ++checks;
    if (!ok)
    {
        std::cout << "FAIL " << what << std::endl;
        std::exit(1);
    }
}

// a heap copy of exactly s.size() bytes: a read beyond the buffer is the sanitizer's to report
gnhost::GenomeCut cut_of(const std::string& s, bool eof)
{
    std::unique_ptr<uint8_t[]> b(new uint8_t[s.size()]);
    std::memcpy(b.get(), s.data(), s.size());
    return gnhost::genome_cut(b.get(), s.size(), eof);
}

void cut_is(const std::string& name, const std::string& s, bool eof, bool ok, uint64_t cut, bool open)
{
    const gnhost::GenomeCut c = cut_of(s, eof);
    expect(c.ok == ok && (!ok || (c.cut == cut && c.open == open)),
           name + ": ok " + std::to_string(c.ok) + " cut " + std::to_string(c.cut) + " open " + std::to_string(c.open));
}

// the record rules, restated: the first line is the header; in the others isspace bytes and digits are skipped, the dna15 letters of
// either case are kept, anything else is illegal
bool letters_restated(const std::string& rec, std::string& out)
{
    out.clear();
    size_t at = rec.find('\n');
    if (at == std::string::npos)
        return true;
    for (++at; at < rec.size(); ++at)
    {
        const unsigned char c = (unsigned char)rec[at];
        const bool space = c == ' ' || (c >= 9 && c <= 13), digit = c >= '0' && c <= '9';
        if (space || digit)
            continue;
        const unsigned char u = (unsigned char)(c & ~0x20);
        const bool alpha = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
        if (!alpha || u == 'E' || u == 'F' || u == 'I' || u == 'J' || u == 'L' || u == 'O' || u == 'P' || u == 'Q' || u == 'X' || u == 'Z')
            return false;
        out.push_back((char)c);
    }
    return true;
}

void letters_agree(const std::string& rec)
{
    std::unique_ptr<uint8_t[]> b(new uint8_t[rec.size() ? rec.size() : 1]);
    std::memcpy(b.get(), rec.data(), rec.size());
    std::string got, want;
    const bool  a = gnhost::genome_record_letters(b.get(), rec.size(), got), c = letters_restated(rec, want);
    expect(a == c && (!a || got == want), "letters of a record of " + std::to_string(rec.size()) + " bytes");
}

} // namespace

int main()
{
    // ---- the cut rule
    cut_is("header at offset 0 only", ">a\nACGT\nACGT\nAC", false, true, 13, true);
    cut_is("header at offset 0 only, newline last", ">a\nACGT\nACGT\n", false, true, 13, true);
    cut_is("header at offset 0 only, its line alone", ">a b c\n", false, true, 7, true);
    cut_is("two headers", ">a\nACGT\n>b\nAC\nGT", false, true, 8, false);
    cut_is("three headers: the last one", ">a\nACGT\n>b\nAC\n>c\nGT\n", false, true, 14, false);
    cut_is("newline and '>' as the last two bytes", ">a\nACGT\n>", false, true, 8, false);
    cut_is("newline and ';' as the last two bytes", ">a\nACGT\n;", false, true, 8, false);
    cut_is("no newline", ">a long header line", false, false, 0, false);
    cut_is("no newline, letters", "ACGTACGT", false, false, 0, false);
    cut_is("empty buffer", "", false, false, 0, false);
    cut_is("end of file without a newline", ">a\nACGT\n>b\nACG", true, true, 14, false);
    cut_is("end of file, no newline at all", ">a", true, true, 2, false);
    cut_is("end of file, empty", "", true, true, 0, false);
    cut_is("';' headers", ";a\nACGT\n;b\nAC\nGT\n", false, true, 8, false);
    cut_is("';' header at offset 0 only", ";a\nAC\nGT\n", false, true, 9, true);
    cut_is("'>' inside a header line", ">a >b >c\nACGT\nAC", false, true, 14, true);
    cut_is("'>' inside the second header line", ">a\nAC\n>b >c;d\nACGT\n", false, true, 6, false);
    cut_is("'>' inside a sequence line is no header", ">a\nAC>GT\nAC;GT\n", false, true, 15, true);
    cut_is("no header at all (the middle of a record)", "ACGT\nACGT\nAC", false, true, 10, true);
    cut_is("a header line first in the middle of a record's chunk", "ACGT\n>b\nAC", false, true, 5, false);
    cut_is("blank lines before a header", ">a\nAC\n\n\n>b\nAC\n", false, true, 8, false);
    cut_is("CRLF", ">a\r\nAC\r\n>b\r\nAC\r\n", false, true, 8, false);
    {
        // a long buffer: the last header is found wherever it lies, and without one the cut is behind the last newline
        std::mt19937 rng(7);
        for (int round = 0; round < 200; ++round)
        {
            std::string s = ">r\n";
            size_t      last_header = 0, last_nl = 2;
            const int   lines = 1 + (int)(rng() % 40);
            for (int l = 0; l < lines; ++l)
            {
                if (rng() % 7 == 0)
                {
                    last_header = s.size();
                    s += rng() % 2 ? ">h >x\n" : ";h\n";
                }
                else
                    s += std::string(1 + rng() % 80, "ACGT"[rng() % 4]) + "\n";
                last_nl = s.size() - 1;
            }
            s += std::string(rng() % 30, 'A'); // an unfinished line
            const gnhost::GenomeCut c = cut_of(s, false);
            expect(c.ok && c.cut == (last_header ? last_header : last_nl + 1) && c.open == (last_header == 0), "random buffer " + std::to_string(round));
        }
    }
    // ---- the letters of a short record
    letters_agree(">a\nACGT\n");
    letters_agree(">a");
    letters_agree(">a\n");
    letters_agree(";a ACGT\nAC GT\t12 acgtn\r\nRYKM\n\n\nSWBDHVNU\n");
    letters_agree(">a\nAC!GT\n");
    letters_agree(">a\nACEGT\n");
    letters_agree(">a\nAC>GT\n");
    letters_agree(std::string(">a\nAC\0GT\n", 9));
    letters_agree(">a\nAC\xc1GT\n");
    letters_agree(">a!E\xff\n  1 ACGT\v\f\n");
    {
        std::mt19937 rng(9);
        for (int round = 0; round < 300; ++round)
        {
            std::string rec = ">h\n";
            const int   n   = (int)(rng() % 60);
            for (int i = 0; i < n; ++i)
            {
                const unsigned r = rng() % 100;
                rec += r < 70 ? "ACGTNacgtnRYKMSWBDHVU"[rng() % 21] : r < 90 ? " \t\n\r\v\f0123456789"[rng() % 16] : (char)(rng() % 256);
            }
            letters_agree(rec);
        }
    }
    std::cout << "ok " << checks << " checks" << std::endl;
    return 0;
}
