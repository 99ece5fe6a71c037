// The element rules of Arith and Math on sparse operands (src/SparseVec_Arith.c, src/SparseVec_Math.c of the
// reference; R's arithmetic.c for the operators), of Compare and Logic, of subassignment, and of pmin / pmax and is.na /
// is.nan / is.infinite, each stated once for the device kernels (kernels_arith.hip) and for a host program
// (tests/arith_rules_main.cpp, compare_rules_main.cpp, assign_rules_main.cpp, sweep_rules_main.cpp,
// pminmax_rules_main.cpp): plain C++, no HIP header needed.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/svt_hip.h"

#ifdef __HIPCC__
#define SVT_HD __host__ __device__
#else
#define SVT_HD
#endif

#define SVT_NA_INT (-2147483647 - 1)

SVT_HD inline double svt_rule_bits(unsigned long long u)
{
	union { unsigned long long u; double d; } x;
	x.u = u;
	return x.d;
}
SVT_HD inline double svt_rule_na_real() { return svt_rule_bits(0x7FF00000000007A2ULL); }   // NA_real_
SVT_HD inline double svt_rule_nan() { return svt_rule_bits(0x7FF8000000000000ULL); }       // R_NaN
SVT_HD inline double svt_rule_inf() { return svt_rule_bits(0x7FF0000000000000ULL); }

// as.double() of an integer
SVT_HD inline double svt_rule_as_double(int32_t x) { return x == SVT_NA_INT ? svt_rule_na_real() : (double) x; }
SVT_HD inline double svt_rule_as_double(double x) { return x; }

// integer op integer for + - * %% %/%: NA propagates; + - * are done in double, a result <= INT_MIN or > INT_MAX is NA
// and raises *ovflow; %% takes the sign of the divisor, %/% floors, a zero divisor gives NA
SVT_HD inline int32_t svt_rule_arith_int(int op, int32_t x, int32_t y, int *ovflow)
{
	if (x == SVT_NA_INT || y == SVT_NA_INT)
		return SVT_NA_INT;
	double vv;
	switch (op) {
	case SVT_ARITH_ADD: vv = (double) x + (double) y; break;
	case SVT_ARITH_SUB: vv = (double) x - (double) y; break;
	case SVT_ARITH_MULT: vv = (double) x * (double) y; break;
	case SVT_ARITH_MOD: {
		if (y == 0) return SVT_NA_INT;
		if (y == -1) return 0;                      // (INT_MIN is NA: no other x overflows, but the C % may trap)
		int32_t zz = x % y;
		if ((y > 0 && zz < 0) || (y < 0 && zz > 0)) zz += y;
		return zz;
	}
	case SVT_ARITH_IDIV: {
		if (y == 0) return SVT_NA_INT;
		if (y == -1) return -x;
		int32_t zz = x / y;
		if (((y > 0 && x < 0) || (y < 0 && x > 0)) && zz * y != x) zz--;
		return zz;
	}
	default:
		return SVT_NA_INT;
	}
	if (vv <= -2147483648.0 || vv > 2147483647.0) {
		*ovflow = 1;
		return SVT_NA_INT;
	}
	return (int32_t) vv;
}

// x ^ y: 1 for x == 1 or y == 0; NaN for a NaN y, for x < 0 with an infinite y, for x == -Inf with a non-integer y; a
// NaN x comes back as x + y, as R_pow does it (arithmetic.c), so that an NA stays an NA whatever pow() makes of one
SVT_HD inline double svt_rule_pow(double x, double y)
{
	if (x == 1.0 || y == 0.0)
		return 1.0;
	if (x != x && y == y)
		return x + y;
	if (y != y || (x < 0.0 && (y == svt_rule_inf() || y == -svt_rule_inf())) || (x == -svt_rule_inf() && y != trunc(y)))
		return svt_rule_nan();
	return pow(x, y);
}

// x %% y = x - y * floor(x / y), with the zero and the infinite cases
SVT_HD inline double svt_rule_mod(double x, double y)
{
	const double inf = svt_rule_inf();
	if (y == 0.0 || x == inf || x == -inf)
		return svt_rule_nan();
	if (x == 0.0)
		return y != y ? y : 0.0;
	if (y == inf)
		return (x != x || x > 0) ? x : inf;
	if (y == -inf)
		return (x != x || x < 0) ? x : -inf;
	return x - y * floor(x / y);
}

// x %/% y = floor(x / y), with the infinite cases
SVT_HD inline double svt_rule_idiv(double x, double y)
{
	const double inf = svt_rule_inf();
	if (y == inf) {
		if (x == -inf) return svt_rule_nan();
		if (x < 0) return -1.0;
	} else if (y == -inf) {
		if (x == inf) return svt_rule_nan();
		if (x > 0) return -1.0;
	}
	return floor(x / y);
}

SVT_HD inline double svt_rule_arith_double(int op, double x, double y)
{
	switch (op) {
	case SVT_ARITH_ADD: return x + y;
	case SVT_ARITH_SUB: return x - y;
	case SVT_ARITH_MULT: return x * y;
	case SVT_ARITH_DIV: return x / y;
	case SVT_ARITH_POW: return svt_rule_pow(x, y);
	case SVT_ARITH_MOD: return svt_rule_mod(x, y);
	case SVT_ARITH_IDIV: return svt_rule_idiv(x, y);
	}
	return svt_rule_nan();
}

// ---- log1p ----
// The device library's log1p is within one ulp of the exact value, not the nearest double: on 8747 ordinary arguments
// 49 results were the neighbour (tests/test_hip_chains.py).  This one computes log(1 + x) in pairs of doubles (a value is
// h + l, |l| <= ulp(h) / 2; error-free sums and fma products, Dekker / Knuth) to about 2^-95 and rounds once:
//   1 + x = 2^e (m + ml), m in [0.75, 1.5) -- exact: the rounding error of 1 + x is kept in ml;
//   r = (m + ml) c - 1 for the tabulated c next to 1 / m, |r| < 2^-7.5, exact up to 2^-106 (c = 1 around m = 1: r = x);
//   log(1 + x) = e log(2) - log(c) + (r - r^2 / 2 + ... + r^16 / 16)        (the first term left out: 2^-121).
// Every other argument -- a NaN, x <= -1, +Inf -- is the library's as before, and so is |x| < 2^-54 (below).
struct svt_dd { double h, l; };
SVT_HD inline svt_dd svt_dd_sum(double a, double b)             // a + b exactly
{
	const double s = a + b, bb = s - a;
	return svt_dd{ s, (a - (s - bb)) + (b - bb) };
}
SVT_HD inline svt_dd svt_dd_sum_ordered(double a, double b)     // the same for |a| >= |b|
{
	const double s = a + b;
	return svt_dd{ s, b - (s - a) };
}
SVT_HD inline svt_dd svt_dd_add(svt_dd a, svt_dd b)
{
	const svt_dd s = svt_dd_sum(a.h, b.h);
	return svt_dd_sum_ordered(s.h, s.l + (a.l + b.l));
}
SVT_HD inline svt_dd svt_dd_mul(svt_dd a, svt_dd b)
{
	const double p = a.h * b.h;
	return svt_dd_sum_ordered(p, fma(a.h, b.h, -p) + (a.h * b.l + a.l * b.h));
}

// c = the double nearest 1 / (0.75 + j / 128); (lh, ll) = -log(c): lh the nearest double, ll the nearest double of the rest
static constexpr double svt_log1p_c[97] = {
	0x1.5555555555555p+0, 0x1.51d07eae2f815p+0, 0x1.4e5e0a72f0539p+0, 0x1.4afd6a052bf5bp+0, 0x1.47ae147ae147bp+0, 0x1.446f86562d9fbp+0, 0x1.4141414141414p+0, 0x1.3e22cbce4a902p+0, 0x1.3b13b13b13b14p+0, 0x1.3813813813814p+0, 0x1.3521cfb2b78c1p+0, 0x1.323e34a2b10bfp+0, 0x1.2f684bda12f68p+0, 0x1.2c9fb4d812ca0p+0, 0x1.29e4129e4129ep+0, 0x1.27350b8812735p+0, 0x1.2492492492492p+0, 0x1.21fb78121fb78p+0, 0x1.1f7047dc11f70p+0, 0x1.1cf06ada2811dp+0, 0x1.1a7b9611a7b96p+0, 0x1.1811811811812p+0, 0x1.15b1e5f75270dp+0, 0x1.135c81135c811p+0, 0x1.1111111111111p+0, 0x1.0ecf56be69c90p+0, 0x1.0c9714fbcda3bp+0, 0x1.0a6810a6810a7p+0, 0x1.0842108421084p+0, 0x1.0624dd2f1a9fcp+0, 0x1.0410410410410p+0, 0x1.0204081020408p+0, 0x1.0000000000000p+0, 0x1.fc07f01fc07f0p-1, 0x1.f81f81f81f820p-1, 0x1.f44659e4a4271p-1, 0x1.f07c1f07c1f08p-1, 0x1.ecc07b301ecc0p-1, 0x1.e9131abf0b767p-1, 0x1.e573ac901e574p-1, 0x1.e1e1e1e1e1e1ep-1, 0x1.de5d6e3f8868ap-1, 0x1.dae6076b981dbp-1, 0x1.d77b654b82c34p-1, 0x1.d41d41d41d41dp-1, 0x1.d0cb58f6ec074p-1, 0x1.cd85689039b0bp-1, 0x1.ca4b3055ee191p-1, 0x1.c71c71c71c71cp-1, 0x1.c3f8f01c3f8f0p-1, 0x1.c0e070381c0e0p-1, 0x1.bdd2b899406f7p-1, 0x1.bacf914c1bad0p-1, 0x1.b7d6c3dda338bp-1, 0x1.b4e81b4e81b4fp-1, 0x1.b2036406c80d9p-1, 0x1.af286bca1af28p-1, 0x1.ac5701ac5701bp-1, 0x1.a98ef606a63bep-1, 0x1.a6d01a6d01a6dp-1, 0x1.a41a41a41a41ap-1, 0x1.a16d3f97a4b02p-1, 0x1.9ec8e951033d9p-1, 0x1.9c2d14ee4a102p-1, 0x1.999999999999ap-1, 0x1.970e4f80cb872p-1, 0x1.948b0fcd6e9e0p-1, 0x1.920fb49d0e229p-1, 0x1.8f9c18f9c18fap-1, 0x1.8d3018d3018d3p-1, 0x1.8acb90f6bf3aap-1, 0x1.886e5f0abb04ap-1, 0x1.8618618618618p-1, 0x1.83c977ab2beddp-1, 0x1.8181818181818p-1, 0x1.7f405fd017f40p-1, 0x1.7d05f417d05f4p-1, 0x1.7ad2208e0ecc3p-1, 0x1.78a4c8178a4c8p-1, 0x1.767dce434a9b1p-1, 0x1.745d1745d1746p-1, 0x1.724287f46debcp-1, 0x1.702e05c0b8170p-1, 0x1.6e1f76b4337c7p-1, 0x1.6c16c16c16c17p-1, 0x1.6a13cd1537290p-1, 0x1.6816816816817p-1, 0x1.661ec6a5122f9p-1, 0x1.642c8590b2164p-1, 0x1.623fa77016240p-1, 0x1.6058160581606p-1, 0x1.5e75bb8d015e7p-1, 0x1.5c9882b931057p-1, 0x1.5ac056b015ac0p-1, 0x1.58ed2308158edp-1, 0x1.571ed3c506b3ap-1, 0x1.5555555555555p-1
};
static constexpr double svt_log1p_l[97][2] = {
	{ -0x1.269621134db91p-2, -0x1.e0efadd9db02ap-56 },
	{ -0x1.1bf99635a6b95p-2, 0x1.e9575c2124912p-56 },
	{ -0x1.1178e8227e47ap-2, -0x1.b8ce2d07f1cb7p-56 },
	{ -0x1.07138604d5864p-2, 0x1.24e912b16ec8bp-60 },
	{ -0x1.f991c6cb3b37ap-3, -0x1.ecca0cdf30143p-58 },
	{ -0x1.e530effe71013p-3, 0x1.f7627ef82f3f0p-57 },
	{ -0x1.d1037f2655e7bp-3, 0x1.3f3adb7b71cbcp-58 },
	{ -0x1.bd087383bd8aap-3, 0x1.1165504ad749ep-59 },
	{ -0x1.a93ed3c8ad9e5p-3, -0x1.bcafa9de97202p-57 },
	{ -0x1.95a5adcf70182p-3, -0x1.8a16283fdbd1cp-57 },
	{ -0x1.823c16551a3c0p-3, -0x1.6dcd318f4187ep-57 },
	{ -0x1.6f0128b756ab9p-3, 0x1.37967087859b9p-59 },
	{ -0x1.5bf406b543db0p-3, 0x1.1f5b44c0df7f7p-61 },
	{ -0x1.4913d8333b563p-3, 0x1.0d5604930f137p-58 },
	{ -0x1.365fcb0159014p-3, -0x1.bea08d2dca256p-57 },
	{ -0x1.23d712a49c201p-3, -0x1.51c7e9efae297p-57 },
	{ -0x1.1178e8227e47ap-3, 0x1.0e63a5f01c693p-58 },
	{ -0x1.fe89139dbd565p-4, 0x1.ac9f4215f9394p-58 },
	{ -0x1.da7276384469ep-4, -0x1.401fa71733017p-58 },
	{ -0x1.b6ac88dad5b1dp-4, 0x1.002bf768e52d0p-58 },
	{ -0x1.9335e5d594988p-4, 0x1.478a85704ccb7p-58 },
	{ -0x1.700d30aeac0e8p-4, -0x1.a36a677b4c8b2p-59 },
	{ -0x1.4d3115d207eacp-4, -0x1.da7d0b1e10b2fp-60 },
	{ -0x1.2aa04a44717a1p-4, -0x1.aea2c72d05c08p-58 },
	{ -0x1.08598b59e3a06p-4, 0x1.dd7009902bf32p-58 },
	{ -0x1.ccb73cdddb2d0p-5, 0x1.e48fb0500efd5p-59 },
	{ -0x1.894aa149fb34bp-5, 0x1.2ba0b44cfaee5p-59 },
	{ -0x1.466aed42de3f9p-5, 0x1.9badefe942718p-60 },
	{ -0x1.0415d89e74440p-5, -0x1.c05cf1d753621p-59 },
	{ -0x1.8492528c8cac5p-6, 0x1.d192d0619fa68p-60 },
	{ -0x1.0205658935837p-6, -0x1.27c8e8416e717p-60 },
	{ -0x1.010157588de69p-7, -0x1.46662d417cecep-62 },
	{ 0x0.0p+0, 0x0.0p+0 },
	{ 0x1.fe02a6b106799p-8, -0x1.e44b7e3711e7fp-67 },
	{ 0x1.fc0a8b0fc03c4p-7, -0x1.83092c5964281p-62 },
	{ 0x1.7b91b07d5b126p-6, -0x1.6d80ab38e9430p-62 },
	{ 0x1.f829b0e7832f8p-6, 0x1.33e3f04f1ef25p-60 },
	{ 0x1.39e87b9febd68p-5, -0x1.5bfa937f551b7p-59 },
	{ 0x1.77458f632dcffp-5, 0x1.8d3ca87b92968p-63 },
	{ 0x1.b42dd711971b9p-5, 0x1.0a34531f67db5p-59 },
	{ 0x1.f0a30c01162a8p-5, 0x1.85f325c5bbacdp-59 },
	{ 0x1.16536eea37ae3p-4, 0x1.2189705cf74cap-58 },
	{ 0x1.341d7961bd1d0p-4, -0x1.3599f227becbbp-58 },
	{ 0x1.51b073f06183cp-4, -0x1.5b61c65e5741ap-58 },
	{ 0x1.6f0d28ae56b4ep-4, -0x1.20db323097324p-59 },
	{ 0x1.8c345d6319b23p-4, -0x1.294d2f5668495p-58 },
	{ 0x1.a926d3a4ad562p-4, -0x1.d7a16eab1e2adp-59 },
	{ 0x1.c5e548f5bc743p-4, 0x1.2eb0bf7c0b0d9p-59 },
	{ 0x1.e27076e2af2eap-4, -0x1.61578001e015ap-60 },
	{ 0x1.fec9131dbeabcp-4, -0x1.5746b9981b36cp-58 },
	{ 0x1.0d77e7cd08e5bp-3, 0x1.9a5dc5e9030adp-57 },
	{ 0x1.1b72ad52f67a2p-3, -0x1.fbe7ee5c69946p-57 },
	{ 0x1.29552f81ff521p-3, 0x1.301771c407dc0p-57 },
	{ 0x1.371fc201e8f75p-3, 0x1.e6cb62af18a02p-62 },
	{ 0x1.44d2b6ccb7d1cp-3, 0x1.7d3d950f87e23p-59 },
	{ 0x1.526e5e3a1b438p-3, -0x1.546ff8a470d3ap-57 },
	{ 0x1.5ff3070a793d6p-3, -0x1.bc60efafc6f6cp-58 },
	{ 0x1.6d60fe719d21bp-3, 0x1.d551d97132e87p-57 },
	{ 0x1.7ab890210d907p-3, -0x1.1072534a57e7dp-57 },
	{ 0x1.87fa06520c911p-3, -0x1.9f7fdbfa08d9ap-57 },
	{ 0x1.9525a9cf456b6p-3, -0x1.26fb3e2b1d1dap-57 },
	{ 0x1.a23bc1fe2b561p-3, 0x1.24dc46c1ea664p-57 },
	{ 0x1.af3c94e80bff3p-3, 0x1.a3398064df33ep-57 },
	{ 0x1.bc286742d8cd4p-3, 0x1.cfce744870f57p-58 },
	{ 0x1.c8ff7c79a9a20p-3, -0x1.4f689f8434011p-57 },
	{ 0x1.d5c216b4fbb94p-3, -0x1.a37794d03657dp-58 },
	{ 0x1.e27076e2af2e8p-3, -0x1.61578001e015ep-59 },
	{ 0x1.ef0adcbdc5935p-3, 0x1.e8637950dc20dp-57 },
	{ 0x1.fb9186d5e3e29p-3, 0x1.355519b0de535p-57 },
	{ 0x1.0402594b4d041p-2, -0x1.08ec217a5022dp-57 },
	{ 0x1.0a324e27390e2p-2, 0x1.bdcfde8061c03p-56 },
	{ 0x1.1058bf9ae4ad4p-2, 0x1.3f415699663ecp-63 },
	{ 0x1.1675cababa60fp-2, 0x1.ce63eab883727p-61 },
	{ 0x1.1c898c16999fbp-2, 0x1.9f1a39d500e3cp-56 },
	{ 0x1.22941fbcf7966p-2, -0x1.dbd7ac258a2bdp-58 },
	{ 0x1.2895a13de86a4p-2, 0x1.7ad24c13f040fp-56 },
	{ 0x1.2e8e2bae11d31p-2, -0x1.1e99b72bd7bf2p-57 },
	{ 0x1.347dd9a987d56p-2, -0x1.16ea62c048cfbp-56 },
	{ 0x1.3a64c556945eap-2, 0x1.cbcd735d03424p-60 },
	{ 0x1.404308686a7e4p-2, -0x1.f79f6c1059cdbp-57 },
	{ 0x1.4618bc21c5ec2p-2, -0x1.7a42642661c62p-61 },
	{ 0x1.4be5f957778a1p-2, -0x1.4b366b609027ap-58 },
	{ 0x1.51aad872df82ep-2, -0x1.d8db0a7cc1543p-56 },
	{ 0x1.5767717455a6cp-2, -0x1.fb2a49af933e8p-57 },
	{ 0x1.5d1bdbf5809cap-2, -0x1.7dc9c7c23801fp-56 },
	{ 0x1.62c82f2b9c796p-2, -0x1.090a0dd59fe35p-58 },
	{ 0x1.686c81e9b14adp-2, 0x1.710af840538e3p-56 },
	{ 0x1.6e08eaa2ba1e4p-2, -0x1.bfb1b39ca3a0fp-56 },
	{ 0x1.739d7f6bbd007p-2, 0x1.ce24c53fad3f0p-58 },
	{ 0x1.792a55fdd47a1p-2, 0x1.f057691fe9ed7p-56 },
	{ 0x1.7eaf83b82afc2p-2, -0x1.698b43096b576p-59 },
	{ 0x1.842d1da1e8b18p-2, 0x1.54ec519784677p-56 },
	{ 0x1.89a3386c1425bp-2, 0x1.2d38c40881e0bp-57 },
	{ 0x1.8f11e873662c8p-2, 0x1.f85da755a61a3p-56 },
	{ 0x1.947941c2116fbp-2, 0x1.1266e8a3e8838p-57 },
	{ 0x1.99d958117e08ap-2, -0x1.315b444ee1f38p-56 },
	{ 0x1.9f323ecbf984dp-2, -0x1.a92e513217f58p-59 },
};
// (-1)^(k + 1) / k for k = 1 .. 16, in the same two parts
static constexpr double svt_log1p_k[16][2] = {
	{ 0x1.0000000000000p+0, 0x0.0p+0 },
	{ -0x1.0000000000000p-1, 0x0.0p+0 },
	{ 0x1.5555555555555p-2, 0x1.5555555555555p-56 },
	{ -0x1.0000000000000p-2, 0x0.0p+0 },
	{ 0x1.999999999999ap-3, -0x1.999999999999ap-57 },
	{ -0x1.5555555555555p-3, -0x1.5555555555555p-57 },
	{ 0x1.2492492492492p-3, 0x1.2492492492492p-57 },
	{ -0x1.0000000000000p-3, 0x0.0p+0 },
	{ 0x1.c71c71c71c71cp-4, 0x1.c71c71c71c71cp-58 },
	{ -0x1.999999999999ap-4, 0x1.999999999999ap-58 },
	{ 0x1.745d1745d1746p-4, -0x1.745d1745d1746p-59 },
	{ -0x1.5555555555555p-4, -0x1.5555555555555p-58 },
	{ 0x1.3b13b13b13b14p-4, -0x1.3b13b13b13b14p-58 },
	{ -0x1.2492492492492p-4, -0x1.2492492492492p-58 },
	{ 0x1.1111111111111p-4, 0x1.1111111111111p-60 },
	{ -0x1.0000000000000p-4, 0x0.0p+0 },
};
// log(2) in three parts, the first with its low 11 bits clear: e * h is exact for |e| < 2048
static constexpr double svt_log1p_ln2[3] = { 0x1.62e42fefa3800p-1, 0x1.ef35793c76730p-45, 0x1.f97b57a079a19p-103 };

SVT_HD inline double svt_rule_log1p(double x)
{
	if (!(x > -1.0) || x == svt_rule_inf())
		return log1p(x);
	const svt_dd u = svt_dd_sum(1.0, x);
	int e;
	double m = frexp(u.h, &e);                              // u.h = m 2^e, m in [0.5, 1)
	if (m < 0.75) { m *= 2.0; e--; }
	const double ml = ldexp(u.l, -e);
	const int j = (int) ((m - 0.75) * 128.0 + 0.5);
	const double c = svt_log1p_c[j], p = m * c;
	const svt_dd r = svt_dd_sum(p - 1.0, fma(m, c, -p) + ml * c);      // (p - 1 is exact: p in [0.5, 2])
	svt_dd s = { svt_log1p_k[15][0], svt_log1p_k[15][1] };
	for (int k = 14; k >= 0; k--)
		s = svt_dd_add(svt_dd{ svt_log1p_k[k][0], svt_log1p_k[k][1] }, svt_dd_mul(r, s));
	s = svt_dd_mul(r, s);
	const double ee = (double) e;
	svt_dd acc = svt_dd_sum(ee * svt_log1p_ln2[0], ee * svt_log1p_ln2[1]);
	acc.l += ee * svt_log1p_ln2[2];
	acc = svt_dd_add(acc, svt_dd{ svt_log1p_l[j][0], svt_log1p_l[j][1] });
	return svt_dd_add(acc, s).h;
}

// the members of the Math group offered here, on a double
SVT_HD inline double svt_rule_math(int op, double x)
{
	switch (op) {
	case SVT_MATH_ABS: return fabs(x);
	case SVT_MATH_SIGN: return x != x ? x : (x > 0.0 ? 1.0 : (x == 0.0 ? 0.0 : -1.0));
	case SVT_MATH_SQRT: return sqrt(x);
	case SVT_MATH_FLOOR: return floor(x);
	case SVT_MATH_CEILING: return ceil(x);
	case SVT_MATH_TRUNC: return trunc(x);
	// below 2^-54 both series round to x itself (|x^2 / 2| < ulp(x) / 4); said here because the device library
	// answers 0 for the smallest denormals, and a zero result is an entry dropped
	case SVT_MATH_LOG1P: return fabs(x) < 0x1p-54 ? x : svt_rule_log1p(x);
	case SVT_MATH_EXPM1: return fabs(x) < 0x1p-54 ? x : expm1(x);
	}
	return svt_rule_nan();
}

// ---- Compare and Logic (src/SparseVec_Compare.c, src/SparseVec_Logic.c of the reference) ----
// x op y for == != <= >= < >: NA when either side is a NaN (NA_real_ included), else 0 or 1.  The operands come
// through svt_rule_as_double, so NA_integer_ arrives as NA_real_.  The reference separates Compare_int_int,
// Compare_int_double and Compare_double_double; this one rule in double is exact for all of them, because every int32
// is a double and the conversion keeps the order: two integers compare in double as they compare as integers.
SVT_HD inline int32_t svt_rule_compare(int op, double x, double y)
{
	if (x != x || y != y)
		return SVT_NA_INT;
	switch (op) {
	case SVT_COMPARE_EQ: return x == y;
	case SVT_COMPARE_NE: return x != y;
	case SVT_COMPARE_LE: return x <= y;
	case SVT_COMPARE_GE: return x >= y;
	case SVT_COMPARE_LT: return x < y;
	case SVT_COMPARE_GT: return x > y;
	}
	return SVT_NA_INT;
}

// x & y, x | y on logical values (0, 1, NA): Logic_int_int.  & is FALSE next to a FALSE, else NA next to an NA; | is
// TRUE next to a TRUE, else NA next to an NA.
SVT_HD inline int32_t svt_rule_logic(int op, int32_t x, int32_t y)
{
	if (op == SVT_LOGIC_AND) {
		if (x == 0 || y == 0)
			return 0;
		if (x == SVT_NA_INT || y == SVT_NA_INT)
			return SVT_NA_INT;
		return 1;
	}
	if (x == 1 || y == 1)                               // SVT_LOGIC_OR
		return 1;
	if (x == SVT_NA_INT || y == SVT_NA_INT)
		return SVT_NA_INT;
	return 0;
}

// ---- sweep(x, MARGIN, STATS, op): x op STATS[k], one element of a vector per row or per leaf ----
// Whether the element `s` of a vector of type s_Rtype keeps `x op s` sparse, i.e. whether 0 op s is zero (FALSE): the
// scalar conditions of .Arith_SVT1_v2 and .Compare_SVT1_v2 (R/SparseArray-Arith-methods.R:113-124,
// R/SparseArray-Compare-methods.R:75-112), asked of every element.  An integer or logical element arrives as its double
// value, INT_MIN standing for NA, as the scalar of the maps does.
SVT_HD inline double svt_rule_element(double s, int s_Rtype)
{
	return s_Rtype != SVT_REALSXP && s == -2147483648.0 ? svt_rule_na_real() : s;
}
// *: not NA / NaN and finite; / %% %/%: not NA / NaN and != 0; ^: not NA / NaN and > 0; + and -: no element does
SVT_HD inline bool svt_rule_arith_keeps_sparse(int op, double s, int s_Rtype)
{
	const double v = svt_rule_element(s, s_Rtype);
	if (v != v)
		return false;
	switch (op) {
	case SVT_ARITH_MULT: return v != svt_rule_inf() && v != -svt_rule_inf();
	case SVT_ARITH_DIV:
	case SVT_ARITH_MOD:
	case SVT_ARITH_IDIV: return v != 0.0;
	case SVT_ARITH_POW: return v > 0.0;
	}
	return false;
}
// not NA / NaN, and 0 op s is FALSE
SVT_HD inline bool svt_rule_compare_keeps_sparse(int op, double s, int s_Rtype)
{
	return svt_rule_compare(op, 0.0, svt_rule_element(s, s_Rtype)) == 0;
}

// ---- subassignment x[i, j] <- value (src/SparseArray_subassignment.c of the reference) ----
// a value in the result's type: the same type moves as bits, int32 -> double converts and NA_integer_ becomes NA_real_
SVT_HD inline void svt_rule_widen(int32_t v, int32_t *out) { *out = v; }
SVT_HD inline void svt_rule_widen(double v, double *out) { *out = v; }
SVT_HD inline void svt_rule_widen(int32_t v, double *out) { *out = svt_rule_as_double(v); }

// ---- pmin(x, y) / pmax(x, y) (.pminmax2, R/SparseArray-misc-methods.R:111-137 of the reference) ----
// is.na() of a value: a NaN (NA_real_ is one) for a double, NA_integer_ for an integer or a logical
SVT_HD inline bool svt_rule_isna(double v) { return v != v; }
SVT_HD inline bool svt_rule_isna(int32_t v) { return v == SVT_NA_INT; }
// One cell of .pminmax2 on two values already widened to the result's type (svt_rule_widen), op SVT_PMINMAX_MIN or _MAX.
// Its five steps are ans <- x; ans[nzwhich(y < x)] <- y (nzwhich takes an NA for a nonzero, so an NA on either side puts
// y there); then ans[nzwhich(is.na(x))] <- x without na.rm, ans[nzwhich(is.na(y))] <- x with it.  Read for one cell:
// without na.rm an NA x wins, then an NA y, else the comparison; with na.rm an NA y loses to x whatever x is, then an NA
// x loses to y.  Ties take x.  The chosen side comes back as its bits: a NaN keeps its payload, NA_real_ stays NA_real_.
template <typename T>
SVT_HD inline T svt_rule_pminmax(int op, int na_rm, T x, T y)
{
	return svt_rule_isna(na_rm ? y : x) ? x : svt_rule_isna(na_rm ? x : y) ? y : (op == SVT_PMINMAX_MIN ? y < x : y > x) ? y : x;
}
// Whether the scalar or vector element `s` keeps pmin(x, s) / pmax(x, s) sparse, i.e. whether pmin(0, s) == 0: not NA /
// NaN, and >= 0 for pmin, <= 0 for pmax (-0.0 passes both; +Inf passes pmin, -Inf pmax).  `op` may carry
// SVT_PMINMAX_NA_RM: an NA element is refused with na.rm too, pmin(0, NA, na.rm = TRUE) being 0 but pmin(v, NA) v.
SVT_HD inline bool svt_rule_pminmax_keeps_sparse(int op, double s, int s_Rtype)
{
	return (op & ~SVT_PMINMAX_NA_RM) == SVT_PMINMAX_MIN ? svt_rule_element(s, s_Rtype) >= 0.0 : svt_rule_element(s, s_Rtype) <= 0.0;
}

// ---- is.na(x), is.nan(x), is.infinite(x) (C_SVT_apply_isFUN, src/SparseArray_misc_methods.c of the reference) ----
// 1 or 0.  is.na: ISNAN for a double (NA_real_ and every NaN), NA_integer_ for an integer or a logical; is.nan: a NaN
// that is not NA_real_ (R_IsNaN: the low word is not 1954, the test svt_coerce_rules.h states for R_IsNA); is.infinite:
// +-Inf.  An integer or logical value is never NaN or infinite: base R's answer (the reference stops with an internal
// error for such an operand).
SVT_HD inline int32_t svt_rule_isfun(int op, double v)
{
	union { double d; unsigned long long u; } b;
	b.d = v;
	return op == SVT_IS_NA ? v != v : op == SVT_IS_NAN ? v != v && (unsigned int) (b.u & 0xFFFFFFFFu) != 1954u
							   : op == SVT_IS_INFINITE && (v == svt_rule_inf() || v == -svt_rule_inf());
}
SVT_HD inline int32_t svt_rule_isfun(int op, int32_t v) { return op == SVT_IS_NA && v == SVT_NA_INT; }

// One place of x merged with the placed operand Y (the new values of the selected cells that may have to be stored; Y
// has entries in covered leaves only).  in_y: Y stores the place (alone or next to an x entry) -- the result is Y's
// value; else x alone stores it: dropped when its row and its leaf are both covered (the cell was assigned a zero),
// x's value otherwise.  Returns whether the result is stored, *out its value: an entry is kept unless its leaf is
// covered and its value == 0 (-0.0 and integer 0 too; a NaN or NA is kept) -- a selected leaf is rebuilt from its dense
// form, so a stored zero of x in it goes even on a row outside i, while an uncovered leaf keeps every entry as it is.
template <typename TX, typename TY, typename TO>
SVT_HD inline bool svt_rule_assign(bool in_y, TX xv, TY yv, bool row_covered, bool leaf_covered, TO *out)
{
	if (in_y) {
		svt_rule_widen(yv, out);
	} else {
		if (row_covered && leaf_covered)
			return false;
		svt_rule_widen(xv, out);
	}
	return !(leaf_covered && *out == (TO) 0);
}

// ---- subassignment by an L-index or M-index (subassign_leaf_by_OPBuf, src/SparseArray_subassignment.c) ----
// One place of x merged with the placed operand Y of kernels_lindex.hip: Y holds one entry per assigned cell, the
// cell's last value, a zero too.  in_y: Y stores the place -- the result is Y's value widened, stored iff it is not
// zero (-0.0 and integer 0 are zero; a NaN or NA is stored).  Else x alone stores it: no index reached the cell, and
// the entry stays as it is, a stored zero included.  There are no cover tables.
template <typename TX, typename TY, typename TO>
SVT_HD inline bool svt_rule_assign_cells(bool in_y, TX xv, TY yv, TO *out)
{
	if (in_y) {
		svt_rule_widen(yv, out);
		return !(*out == (TO) 0);
	}
	svt_rule_widen(xv, out);
	return true;
}

// the wider of two types, logical < integer < double; 0 when either is none of them
SVT_HD inline int svt_rule_assign_out_Rtype(int x_Rtype, int v_Rtype)
{
	const bool xo = x_Rtype == SVT_LGLSXP || x_Rtype == SVT_INTSXP || x_Rtype == SVT_REALSXP;
	const bool vo = v_Rtype == SVT_LGLSXP || v_Rtype == SVT_INTSXP || v_Rtype == SVT_REALSXP;
	if (!xo || !vo) return 0;
	if (x_Rtype == SVT_REALSXP || v_Rtype == SVT_REALSXP) return SVT_REALSXP;
	return x_Rtype == SVT_INTSXP || v_Rtype == SVT_INTSXP ? SVT_INTSXP : SVT_LGLSXP;
}

// the type of the result (SVT_INTSXP / SVT_REALSXP), or 0 for a combination that is not offered
SVT_HD inline int svt_rule_out_Rtype(int kind, int op, int x_Rtype, int y_Rtype)
{
	const bool xi = x_Rtype == SVT_INTSXP, xd = x_Rtype == SVT_REALSXP;
	const bool yi = y_Rtype == SVT_INTSXP, yd = y_Rtype == SVT_REALSXP;
	switch (kind) {
	case SVT_ARITH_MERGE:
		if (!(xi || xd) || !(yi || yd) || op < SVT_ARITH_ADD || op > SVT_ARITH_MULT) return 0;
		return xi && yi ? SVT_INTSXP : SVT_REALSXP;
	case SVT_ARITH_SCALAR:
		if (!(xi || xd) || !(yi || yd) || op < SVT_ARITH_MULT || op > SVT_ARITH_IDIV) return 0;
		return xi && yi && op != SVT_ARITH_DIV && op != SVT_ARITH_POW ? SVT_INTSXP : SVT_REALSXP;
	case SVT_ARITH_NEG:
		return xi || xd ? x_Rtype : 0;
	case SVT_ARITH_MATH:
		return xd && op >= SVT_MATH_ABS && op <= SVT_MATH_EXPM1 ? SVT_REALSXP : 0;
	}
	return 0;
}
