// Driver of tests/test_carve_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_carve.h alone (no HIP), with the address
// and undefined-behaviour sanitizers. Every line of standard input is one carve: the sizes of its pieces in bytes, in the order
// they are taken (an empty line: no piece). The answer to each is one line: the offset of every piece, then bytes and counted.
#include "rtk_carve.h"

#include <iostream>
#include <sstream>
#include <string>

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		Carve c;
		unsigned long long piece;
		while (in >> piece) std::cout << c.take((size_t)piece) << ' ';
		if (!in.eof()) { std::cerr << "bad line: " << line << "\n"; return 2; }
		std::cout << c.bytes << ' ' << c.counted << "\n";
	}
	return 0;
}
