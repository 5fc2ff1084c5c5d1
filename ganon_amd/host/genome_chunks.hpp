// genome_chunks.hpp -- the host's share of `ganon-build --parse device` (hasher.hpp: Hasher::hash_text_file): which files travel as text,
// where a buffer of genome text is cut into the chunks the device tokenises (csrc/gn_genome.hip), and the letters of a record too short
// for the device's pieces.  Pure host code, no HIP: tests/genome_chunks_driver.cpp runs it under the sanitizers.
#pragma once

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace gnhost
{

struct GenomeCut
{
    uint64_t cut  = 0;     // the chunk is text[0, cut)
    bool     open = false; // it ends inside its last record (GN_GENOME_OPEN_END): the cut lies behind a newline, not before a header
    bool     ok   = false; // false: no newline in the buffer -- the file goes to the sequential reader
};

// text[0] is the first byte of a line; `eof`: the file ends with the buffer.  At the end of the file the chunk is the buffer.  Otherwise
// it ends before the last line that begins a record behind offset 0 ("\n>" or "\n;"): everything before it is whole records.  Without
// such a line it ends behind the last newline, inside a record.
inline GenomeCut genome_cut(const uint8_t* text, uint64_t n, bool eof)
{
    if (eof)
        return { n, false, true };
    const uint8_t* last = nullptr; // the buffer's last newline
    for (uint64_t end = n; end > 0;)
    {
        const uint8_t* nl = static_cast<const uint8_t*>(memrchr(text, '\n', end));
        if (!nl)
            break;
        if (!last)
            last = nl;
        const uint64_t next = (uint64_t)(nl - text) + 1;
        if (next < n && (text[next] == '>' || text[next] == ';'))
            return { next, false, true };
        end = next - 1;
    }
    if (!last)
        return { 0, false, false };
    return { (uint64_t)(last - text) + 1, true, true };
}

// The letters of the record whose text is rec[0, n): a header line, then its sequence lines up to the next record (SeqReader::next's
// character-wise path: isspace bytes and digits are skipped).  false on a byte that is no dna15 letter.
inline bool genome_record_letters(const uint8_t* rec, uint64_t n, std::string& out)
{
    static const char* kLetters = "ABCDGHKMNRSTUVWYabcdghkmnrstuvwy";
    out.clear();
    const uint8_t* p = static_cast<const uint8_t*>(std::memchr(rec, '\n', n));
    if (!p)
        return true; // (the header line alone)
    for (++p; p < rec + n; ++p)
    {
        const unsigned char c = *p;
        if (std::isspace(c) || std::isdigit(c))
            continue;
        if (c == 0 || !std::strchr(kLetters, c))
            return false;
        out.push_back((char)c);
    }
    return true;
}

// Does the file travel as text?  FASTA by its name (the extensions SeqReader knows), plain or one gzip stream; bzip2, blocked gzip (its
// members are inflated in parallel by the sequential reader's source) and names that are FASTQ stay on the host path.
inline bool genome_text_eligible(const std::string& path)
{
    auto ends = [](const std::string& s, const char* e) {
        const size_t n = std::strlen(e);
        return s.size() >= n && s.compare(s.size() - n, n, e) == 0;
    };
    std::string base = path;
    for (const char* z : { ".gz", ".bgzf", ".bgz" })
        if (ends(base, z))
        {
            base.resize(base.size() - std::strlen(z));
            break;
        }
    bool fasta = false;
    for (const char* e : { ".fa", ".fasta", ".fna", ".ffn", ".faa", ".frn", ".fas" })
        fasta = fasta || ends(base, e);
    if (!fasta)
        return false;
    unsigned char h[18] = { 0 };
    std::FILE*    f     = std::fopen(path.c_str(), "rb");
    if (!f)
        return false;
    const size_t got = std::fread(h, 1, sizeof(h), f);
    std::fclose(f);
    // BGZF: a gzip member with an extra field whose first subfield is 'B' 'C'
    const bool bgzf = got == sizeof(h) && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[12] == 'B' && h[13] == 'C';
    return !bgzf;
}

} // namespace gnhost
